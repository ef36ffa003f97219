"""Vocabulary sets for czc_generate_rows_vocab (include/conzic_hip.h): host-side tables, the counterpart of rivals.py and draws.py.

A set is a bitset over the BERT vocabulary, uint32 [W] with W = ceil(V / 32): bit (i & 31) of word (i >> 5) is 1 when id i is
allowed.  A call carries a table uint32 [n_sets, W] and an index per row (-1 = no set); in a row's masked softmax the mask factor
of id i is token_mask[i] * bit(i), the '.' rule still on top.  `pack` builds tables from id lists or boolean masks, `ban` / `allow`
build one set from words, `effective_size` counts what a set leaves after the token mask, and the rest is the command-line and
runtime plumbing shared by demo_cli and run_cli (--ban_words, --allow_words, --ban_per_sample)."""
import logging
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

_log = logging.getLogger("ConZIC")


def words_per_set(V: int) -> int:
    return (int(V) + 31) // 32


def pack(items, V: int) -> np.ndarray:
    """uint32 [n, W] from n sets, each a boolean mask [V] (True = allowed) or a list of the allowed ids.  Bits at or above V stay 0."""
    V = int(V)
    if V < 1:
        raise ValueError("pack: V must be >= 1")
    W = words_per_set(V)
    out = np.zeros((len(items), W), dtype=np.uint32)
    for n, item in enumerate(items):
        a = np.asarray(item)
        if a.dtype == np.bool_:
            if a.shape != (V,):
                raise ValueError(f"pack: set {n} is a boolean mask of shape {a.shape}, not ({V},)")
            ids = np.nonzero(a)[0]
        else:
            ids = a.astype(np.int64).reshape(-1)
            if ids.size and (ids.min() < 0 or ids.max() >= V):
                raise ValueError(f"pack: set {n} holds an id outside [0, {V})")
        np.bitwise_or.at(out[n], ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)).astype(np.uint32))
    return out


def unpack(bits, V: int) -> np.ndarray:
    """bool [n, V] (or [V] for one set [W]) from bitsets: the inverse of pack; bits at or above V are dropped"""
    b = np.asarray(bits, dtype=np.uint32)
    ids = np.arange(int(V))
    return ((b[..., ids >> 5] >> (ids & 31).astype(np.uint32)) & 1).astype(bool)


def token_ids(tokenizer, words: Sequence[str]) -> Tuple[List[int], List[str]]:
    """(ids, skipped): the id of every word that is exactly ONE regular vocabulary token; every other word -- several word
    pieces, unknown, a special token, empty -- goes to `skipped` and is logged, never silently dropped."""
    special = set(int(i) for i in getattr(tokenizer, "all_special_ids", []))
    unk = getattr(tokenizer, "unk_token_id", None)
    ids, skipped = [], []
    for w in words:
        enc = [int(i) for i in tokenizer.encode(w)]
        if enc and enc[0] == getattr(tokenizer, "cls_token_id", None):
            enc = enc[1:]
        if enc and enc[-1] == getattr(tokenizer, "sep_token_id", None):
            enc = enc[:-1]
        if len(enc) == 1 and enc[0] != unk and enc[0] not in special:
            ids.append(enc[0])
        else:
            skipped.append(w)
    if skipped:
        _log.info(f"vocabulary set: skipped {skipped} (not exactly one vocabulary token)")
    return ids, skipped


def _vocab_size(tokenizer) -> int:
    return int(tokenizer.vocab_size)


def ban(tokenizer, words: Sequence[str]) -> Tuple[np.ndarray, List[str]]:
    """(bits uint32 [W], skipped): every id allowed except those of `words`"""
    V = _vocab_size(tokenizer)
    ids, skipped = token_ids(tokenizer, words)
    m = np.ones((V,), dtype=bool)
    m[ids] = False
    return pack([m], V)[0], skipped


def allow(tokenizer, words: Sequence[str], keep_dot: bool = True) -> Tuple[np.ndarray, List[str]]:
    """(bits uint32 [W], skipped): only the ids of `words` allowed; keep_dot adds '.' (the engine's '.' rule decides about it at
    every position whatever the set says; the bit only matters to effective_size and to readers of the table)"""
    V = _vocab_size(tokenizer)
    ids, skipped = token_ids(tokenizer, words)
    if keep_dot:
        dot = tokenizer.convert_tokens_to_ids(".")
        if dot is not None and dot != getattr(tokenizer, "unk_token_id", None):
            ids = ids + [int(dot)]
    return pack([ids], V)[0], skipped


def effective_size(bits, token_mask):
    """ids a set leaves after the token mask: #{i : bit(i) and token_mask[i] != 0}; int for one set [W], int array [n] for [n, W]"""
    tm = np.asarray(token_mask).reshape(-1) != 0
    n = (unpack(bits, tm.size) & tm).sum(axis=-1)
    return int(n) if np.ndim(n) == 0 else n.astype(np.int64)


# ---- what a runtime call is handed -----------------------------------------------------------------------------------

class Vocab:
    """The `vocab=` argument of runtime.run_generation_samples / caption_samples: `bits` uint32 [n, W] with n = 1 (one set for
    every row) or n = the number of samples (set s for every row of sample s); `allow_list`: the sets are allow-lists, which the
    runtime holds to at least top_k ids after the token mask; `skipped`: per set, the words that were no single token."""

    def __init__(self, bits, allow_list: bool = False, skipped: Optional[Sequence[Sequence[str]]] = None):
        b = np.ascontiguousarray(bits, dtype=np.uint32)
        self.bits = b.reshape(1, -1) if b.ndim == 1 else b
        if self.bits.ndim != 2 or self.bits.shape[0] < 1:
            raise ValueError("Vocab: bits must be uint32 [W] or [n, W]")
        self.allow_list = bool(allow_list)
        self.skipped = [list(s) for s in skipped] if skipped is not None else [[] for _ in range(self.bits.shape[0])]

    def set_of_sample(self, samples_num: int, sample0: int = 0) -> np.ndarray:
        """int32 [samples_num]: the set of sample sample0 + s"""
        n = self.bits.shape[0]
        if n == 1:
            return np.zeros((samples_num,), dtype=np.int32)
        if sample0 + samples_num > n:
            raise ValueError(f"vocab: {n} per-sample sets for samples {sample0}..{sample0 + samples_num - 1}")
        return np.arange(sample0, sample0 + samples_num, dtype=np.int32)

    def check(self, token_mask, top_k: int) -> np.ndarray:
        """the sets' effective sizes; an allow-list below top_k is refused"""
        sizes = np.atleast_1d(effective_size(self.bits, token_mask))
        if self.allow_list and int(sizes.min()) < int(top_k):
            raise ValueError(f"vocab: an allow-list leaves {int(sizes.min())} ids after the token mask, fewer than the {int(top_k)} "
                             "candidates of a step, so [PAD] candidates would be proposed: lower --candidate_k or widen the list")
        return sizes

    def describe(self, token_mask) -> str:
        sizes = np.atleast_1d(effective_size(self.bits, token_mask))
        return " vocab sets: " + "; ".join(f"{i}: {int(n)} ids" + (f", skipped {sk}" if sk else "")
                                           for i, (n, sk) in enumerate(zip(sizes, self.skipped)))


# ---- command line (demo_cli, run_cli) ----------------------------------------------------------------------------------

def parse_words(spec: str) -> List[str]:
    """the words of `spec`: a file with one word per line, else a comma-separated list"""
    if os.path.isfile(spec):
        with open(spec, "r", encoding="utf-8") as f:
            return [w.strip() for w in f if w.strip()]
    return [w.strip() for w in spec.split(",") if w.strip()]


def parse_per_sample(path: str) -> List[List[str]]:
    """--ban_per_sample FILE: line s is the comma-separated ban-list of sample s (an empty line bans nothing)"""
    with open(path, "r", encoding="utf-8") as f:
        return [[w.strip() for w in line.split(",") if w.strip()] for line in f.read().splitlines()]


def add_arguments(p) -> None:
    p.add_argument("--ban_words", type=str, default=None, metavar="FILE|w1,w2,...",
                   help="words no caption may use (a file with one word per line, or a comma-separated list): a vocabulary set "
                        "per row of the engine call on top of the stop-word mask; combines with --batch_samples, --sample_tau and "
                        "--distinct")
    p.add_argument("--allow_words", type=str, default=None, metavar="FILE|w1,w2,...",
                   help="the only words a caption may use (file or comma-separated list; '.' stays allowed); needs at least "
                        "--candidate_k words that survive the stop-word mask; combines with --ban_words (banned words leave the list)")
    p.add_argument("--ban_per_sample", type=str, default=None, metavar="FILE",
                   help="line s of FILE is the comma-separated ban-list of sample s (samples_num lines); requires --batch_samples")


def wanted(a) -> bool:
    return a.ban_words is not None or a.allow_words is not None or a.ban_per_sample is not None


def check_arguments(p, a) -> None:
    """the refused combinations (p.error), after the flags' own parsing"""
    if not wanted(a):
        return
    if a.ban_per_sample is not None and not a.batch_samples:
        p.error("--ban_per_sample gives every sample of one engine call its own list: it requires --batch_samples")
    if getattr(a, "run_type", None) in ("infill", "retrieve"):
        p.error(f"--ban_words / --allow_words / --ban_per_sample do not combine with --run_type {a.run_type} (the engine call "
                "supports vocabulary sets there; the command-line plumbing does not yet)")
    for flag, on in (("--sentence_lens", getattr(a, "sentence_lens", None) is not None),
                     ("--signals", getattr(a, "signals", None) is not None), ("--block_width", getattr(a, "block_width", 1) != 1)):
        if on:
            p.error(f"--ban_words / --allow_words / --ban_per_sample do not combine with {flag} (the engine call supports "
                    "vocabulary sets there; the command-line plumbing does not yet)")
    if a.ban_per_sample is not None:
        if not os.path.isfile(a.ban_per_sample):
            p.error(f"--ban_per_sample: no such file: {a.ban_per_sample}")
        n = len(parse_per_sample(a.ban_per_sample))
        if n != a.samples_num:
            p.error(f"--ban_per_sample: {n} lines for --samples_num {a.samples_num}")


def from_arguments(a, tokenizer) -> Optional[Vocab]:
    """the Vocab of the parsed flags (None: no flag given): one set, or with --ban_per_sample one per sample -- the sample's own
    list on top of --ban_words / --allow_words"""
    if not wanted(a):
        return None
    V = _vocab_size(tokenizer)
    base = np.ones((V,), dtype=bool)
    skipped = []
    if a.allow_words is not None:
        bits, sk = allow(tokenizer, parse_words(a.allow_words))
        base &= unpack(bits, V)
        skipped += sk
    if a.ban_words is not None:
        bits, sk = ban(tokenizer, parse_words(a.ban_words))
        base &= unpack(bits, V)
        skipped += sk
    if a.ban_per_sample is None:
        return Vocab(pack([base], V), allow_list=a.allow_words is not None, skipped=[skipped])
    masks, sks = [], []
    for words in parse_per_sample(a.ban_per_sample):
        bits, sk = ban(tokenizer, words)
        masks.append(base & unpack(bits, V))
        sks.append(skipped + sk)
    return Vocab(pack(masks, V), allow_list=a.allow_words is not None, skipped=sks)
