"""Mixed caption lengths in one batch on czc_generate_rows_len (include/conzic_hip.h): host-side start rows and schedules.

The reference takes one --sentence_len per call.  A row of a czc_generate_rows_len call has its own: row r holds
seed_len + lens[r] + 1 tokens ([CLS] prompt, lens[r] words, [SEP]) in a [R, T] batch whose stride T is the longest row's, the
columns behind them are id 0 ([PAD]) and are never read.  Everything here is NumPy on the host."""
import random as _random
from typing import List, Sequence

import numpy as np

from .native import POS_IDLE

ORDERS = ("sequential", "shuffle")


def _check_lens(lens) -> List[int]:
    out = [int(n) for n in np.asarray(lens).reshape(-1)]
    if not out or any(n < 1 for n in out):
        raise ValueError(f"sentence lengths must be a non-empty list of integers >= 1, got {list(lens)!r}")
    return out


def length_rows(tokenizer, prompt: str, lens: Sequence[int]) -> np.ndarray:
    """Start rows int32 [R, T] for czc_generate_rows_len: row r is the reference's start row at sentence length lens[r]
    (gen_utils.py:56-59, `prompt + [MASK] * len` encoded with [CLS] / [SEP]), padded with id 0 to the longest row's T."""
    lens = _check_lens(lens)
    rows = [np.asarray(tokenizer.encode(prompt + tokenizer.mask_token * n), dtype=np.int32) for n in lens]
    seed_len = len(prompt.split()) + 1
    for row, n in zip(rows, lens):
        if row.size != seed_len + n + 1:
            raise ValueError(f"length_rows: the prompt {prompt!r} does not encode to len(prompt.split()) = {seed_len - 1} tokens")
    out = np.zeros((len(rows), max(r.size for r in rows)), dtype=np.int32)
    for r, row in enumerate(rows):
        out[r, :row.size] = row
    return out


def length_schedules(lens: Sequence[int], order: str, sweeps: int, rng=None):
    """Per-row visiting orders for czc_generate_rows_len.  Sweep s occupies Lmax = max(lens) steps; row r visits its lens[r]
    positions in the sweep's first lens[r] steps -- ascending (`sequential`, gen_utils.py:64-65) or in an order drawn once per row
    and kept for all sweeps (`shuffle`, gen_utils.py:110-115: one `shuffle` of range(lens[r]) per row, in row order, from `rng`;
    None: the process-global `random` stream, as the reference's sample loop draws) -- and is POS_IDLE for the rest of it.  So
    snapshot s is "after sweep s" for every row (gen_utils.py:82-92).  Returns (positions int32 [sweeps * Lmax, R], n_mask
    [sweeps * Lmax], snapshot_every = Lmax)."""
    if order not in ORDERS:
        raise ValueError(f"length order must be sequential|shuffle, got {order!r}")
    lens = _check_lens(lens)
    rng = _random if rng is None else rng
    width = max(lens)
    sweep = np.full((width, len(lens)), POS_IDLE, dtype=np.int32)
    for r, n in enumerate(lens):
        lst = list(range(n))
        if order == "shuffle":
            rng.shuffle(lst)
        sweep[:n, r] = lst
    positions = np.ascontiguousarray(np.tile(sweep, (max(int(sweeps), 0), 1)))
    return positions, [1] * positions.shape[0], width


def trim_rows(ids: np.ndarray, lens: Sequence[int], seed_len: int) -> List[np.ndarray]:
    """The rows of an [R, T] id batch (a snapshot of czc_generate_rows_len) without their padding tails: row r's own
    seed_len + lens[r] + 1 tokens."""
    ids = np.asarray(ids)
    lens = _check_lens(lens)
    if ids.ndim != 2 or ids.shape[0] != len(lens) or ids.shape[1] < seed_len + max(lens) + 1:
        raise ValueError(f"trim_rows: ids {ids.shape} do not hold {len(lens)} rows of up to {seed_len + max(lens) + 1} tokens")
    return [ids[r, :seed_len + n + 1].copy() for r, n in enumerate(lens)]


def decode_rows(tokenizer, ids: np.ndarray, lens: Sequence[int], seed_len: int) -> List[str]:
    """The captions of an [R, T] snapshot as the reference decodes a row of its own length (skip_special_tokens drops [CLS] /
    [SEP]; the padding tail is cut first, so a [PAD] the token mask put INSIDE a caption is treated as the reference treats it)."""
    return [tokenizer.decode([int(t) for t in row], skip_special_tokens=True) for row in trim_rows(ids, lens, seed_len)]
