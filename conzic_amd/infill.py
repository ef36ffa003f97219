"""Infilling, resume and draft polishing on czc_generate_rows_len (include/conzic_hip.h): host-side parsing and schedules.

ConZIC names infilling as one of its control signals: given "a _ dog sitting on a _", only the blanks are polished and the
given words stay as context.  The reference's CLI never exposed it, but its loop body (gen_utils.py:66 `inp[:, seed_len+ii] =
mask`) does it unchanged once every row may start from its own caption and sit out the steps it has no blank for.  This module
turns caption templates into start rows and per-row visiting orders; conzic_amd/runtime.py::run_infill makes the engine calls.
"""
from __future__ import annotations

import random as _random
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .native import POS_IDLE

ORDERS = ("sequential", "shuffle")


def parse_template(tokenizer, prompt: str, text: str, blank: str = "_") -> Tuple[np.ndarray, List[int], int, int]:
    """`[CLS] prompt text [SEP]` with every whitespace-separated `blank` of `text` as exactly one [MASK] token and every other
    word WordPiece-tokenised (a word of several pieces keeps them all).  Returns (ids int32 [T], blank_positions, L, seed_len):
    L = tokens between the prompt and [SEP], seed_len = 1 + tokens of the prompt (gen_utils.py:56 for a prompt of one-piece
    words), blank_positions = ascending positions in [0, L) of the [MASK] tokens (column seed_len + position)."""
    mask = tokenizer.mask_token
    words = [mask if w == blank else w for w in text.split()]
    seed_len = len(tokenizer.encode(prompt)) - 1          # [CLS] + prompt pieces (the trailing [SEP] does not count)
    head = prompt.strip()
    ids = np.asarray(tokenizer.encode((head + " " if head else "") + " ".join(words)), dtype=np.int32)
    T = int(ids.size)
    L = T - seed_len - 1
    if L < 0:
        raise ValueError(f"parse_template: the caption {text!r} tokenises to fewer tokens than the prompt {prompt!r} alone")
    vocab = tokenizer.vocab if hasattr(tokenizer, "vocab") else tokenizer.get_vocab()
    mask_id = int(vocab[mask])
    blanks = [int(p) for p in np.nonzero(ids[seed_len:seed_len + L] == mask_id)[0]]
    return ids, blanks, L, seed_len


def infill_schedules(blank_positions_per_row: Sequence[Sequence[int]], order: str, sweeps: int, rng=None):
    """Per-row visiting orders for czc_generate_rows_from: every sweep visits each row's blanks exactly once, in ascending order
    (`sequential`) or in an order drawn once per row and kept for all sweeps (`shuffle`, as gen_utils.py:110-115 keeps one
    order_list per call): one `shuffle` draw per row, in row order, from `rng` (None: the process-global `random` stream, in
    the style of harness.sample_schedules).  A row with fewer blanks than the longest row is padded with POS_IDLE at the end of
    every sweep.  Returns (positions int32 [n_steps, R], n_mask [n_steps], snapshot_every): n_steps = sweeps x max blanks, one
    snapshot per sweep."""
    if order not in ORDERS:
        raise ValueError(f"infill order must be sequential|shuffle, got {order!r}")
    rng = _random if rng is None else rng
    rows = []
    for blanks in blank_positions_per_row:
        lst = [int(p) for p in blanks]
        if len(set(lst)) != len(lst) or any(p < 0 for p in lst):
            raise ValueError(f"infill_schedules: blank positions must be distinct and >= 0, got {lst}")
        if order == "shuffle":
            rng.shuffle(lst)
        else:
            lst = sorted(lst)
        rows.append(lst)
    R = len(rows)
    width = max((len(r) for r in rows), default=0)
    sweep = np.full((width, max(R, 0)), POS_IDLE, dtype=np.int32)
    for r, lst in enumerate(rows):
        sweep[:len(lst), r] = lst
    positions = np.ascontiguousarray(np.tile(sweep, (max(int(sweeps), 0), 1)))
    return positions, [1] * positions.shape[0], max(width, 1)


def take_rows(positions: np.ndarray, sweeps: int, rows: Sequence[int]):
    """The schedule of a subset of the rows of an infill_schedules result (a group of captions of one length): their columns,
    every sweep cut down to the subset's own longest row.  Returns (positions, n_mask, snapshot_every) as infill_schedules."""
    pos = np.asarray(positions, dtype=np.int32)[:, list(rows)]
    if pos.shape[0] == 0 or sweeps <= 0:
        return np.zeros((0, len(rows)), dtype=np.int32), [], 1
    per = pos.shape[0] // int(sweeps)
    width = int((pos[:per] != POS_IDLE).sum(axis=0).max()) if len(rows) else 0   # the idle padding sits at the end of a sweep
    out = np.ascontiguousarray(pos.reshape(int(sweeps), per, len(rows))[:, :width].reshape(int(sweeps) * width, len(rows)))
    return out, [1] * out.shape[0], max(width, 1)


def group_by_length(parsed: Sequence[Tuple[np.ndarray, List[int], int, int]]) -> Dict[int, List[int]]:
    """Caption indices grouped by token length T, in order of first appearance; the indices of a group ascend.  The order in which
    run_infill logs and returns its captions (it was one engine call per group before czc_generate_rows_len; the call's rows are
    now those of group_for_call)."""
    groups: Dict[int, List[int]] = {}
    for i, (ids, _, _, _) in enumerate(parsed):
        groups.setdefault(int(len(ids)), []).append(i)
    return groups


def group_for_call(parsed: Sequence[Tuple[np.ndarray, List[int], int, int]]) -> Dict[int, List[int]]:
    """The captions of one engine call, keyed by the call's row stride: ONE group with every caption in caption order under the
    longest token length (czc_generate_rows_len gives each row its own length, so token lengths no longer split a call).  The
    captions must share seed_len (one prompt)."""
    if not parsed:
        return {}
    if len({int(p[3]) for p in parsed}) != 1:
        raise ValueError("group_for_call: the captions of a call share one prompt (seed_len)")
    return {max(int(len(p[0])) for p in parsed): list(range(len(parsed)))}


def visit_lists(parsed, positions: str = "blanks") -> List[List[int]]:
    """What each caption's sweep visits: its blanks, or (`all`: polish / resume) every position of the caption."""
    if positions not in ("blanks", "all"):
        raise ValueError(f"positions must be blanks|all, got {positions!r}")
    return [list(blanks) if positions == "blanks" else list(range(L)) for _, blanks, L, _ in parsed]


def last_visited(positions: np.ndarray) -> Optional[int]:
    """The position of the call's last executed row-step (last step, highest row that is not idle), None if nothing ran: where
    utils.update_token_mask leaves the caller's token mask."""
    pos = np.asarray(positions)
    for s in range(pos.shape[0] - 1, -1, -1):
        live = np.nonzero(pos[s] != POS_IDLE)[0]
        if live.size:
            return int(pos[s, live[-1]])
    return None
