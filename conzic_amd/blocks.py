"""Block-synchronous sweeps for czc_generate_rows_tied (include/conzic_hip.h): host-side schedules, the counterpart of
lengths.py and draws.py.  Pure Python / NumPy: no torch, no engine.

A caption of L positions is polished by `width` tied rows (one group).  A sweep's visiting order is cut into
nb = ceil(L / width) BLOCKS; at a step every slot of the group takes one position of the step's block, masked in the
sentence the group held before the step, and all winners are written back together.  A sweep then costs nb serial steps
instead of L, each on a batch `width` times larger.

  block_schedule(order, width)          one sweep's visiting order -> nb consecutive blocks (only the last may be short)
  sequential_order(L, width, layout)    the blocks of a sequential sweep: "interleaved" deals the positions round-robin,
                                        block i = i, i + nb, i + 2 nb, ... (neighbouring words, the most strongly coupled,
                                        never update together; width = ceil(L / 2) is red-black: evens, then odds);
                                        "contiguous" is block i = [i width, (i + 1) width)
  tied_rows(n_captions, width)          row caption * width + slot: groups, caption of row, image of row
  tied_positions(sweeps, width)         [n_steps, width] positions of one caption's slots, CZC_POS_IDLE where a block is
                                        shorter than the width, and snapshot_every = nb
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

POS_IDLE = -1  # include/conzic_hip.h CZC_POS_IDLE (native.POS_IDLE; kept here so that this module needs no library)
LAYOUTS = ("interleaved", "contiguous")


def n_blocks(L: int, width: int) -> int:
    """Serial steps of one sweep: ceil(L / width)."""
    if L < 1 or width < 1:
        raise ValueError(f"blocks: need L >= 1 and width >= 1, got L = {L}, width = {width}")
    return -(-L // width)


def resolve_width(width: int, L: int) -> int:
    """The CLIs' --block_width: 0 means L, anything above L is L."""
    if width < 0:
        raise ValueError(f"block width must be >= 0, got {width}")
    return L if width == 0 or width > L else width


def block_schedule(order: Sequence[int], width: int) -> List[List[int]]:
    """One sweep's visiting order cut into ceil(L / width) consecutive blocks; only the last one may be short."""
    order = [int(p) for p in order]
    n_blocks(len(order), width)
    return [order[i:i + width] for i in range(0, len(order), width)]


def sequential_order(L: int, width: int, layout: str = "interleaved") -> List[List[int]]:
    """The blocks of a sequential sweep.  interleaved: block i holds i, i + nb, i + 2 nb, ... with nb = ceil(L / width), so
    the block sizes fall by at most one from the first block to the last and no block holds two neighbours once nb >= 2.
    contiguous: block i is [i width, (i + 1) width)."""
    nb = n_blocks(L, width)
    if layout == "interleaved":
        return [list(range(i, L, nb)) for i in range(nb)]
    if layout == "contiguous":
        return block_schedule(range(L), width)
    raise ValueError(f"block layout {layout!r}: expected one of {LAYOUTS}")


def _as_blocks(sweep, width: int) -> List[List[int]]:
    sweep = list(sweep)
    if sweep and isinstance(sweep[0], (list, tuple, np.ndarray)):
        return [[int(p) for p in b] for b in sweep]
    return block_schedule(sweep, width)


def tied_positions(orders_per_sweep: Sequence, width: int) -> Tuple[np.ndarray, int]:
    """Positions of one caption's `width` slots over the sweeps.  Every entry of `orders_per_sweep` is one sweep: a flat
    visiting order (cut by block_schedule) or the blocks themselves (sequential_order).  Every sweep must hold each of the L
    positions once and have nb = ceil(L / width) blocks of at most `width` positions.  Returns (int32 [n_sweeps * nb, width]
    with CZC_POS_IDLE in the slots a short block leaves empty, snapshot_every = nb)."""
    rows, nb, L = [], None, None
    for sweep in orders_per_sweep:
        blocks = _as_blocks(sweep, width)
        flat = sorted(p for b in blocks for p in b)
        L = len(flat) if L is None else L
        if flat != list(range(L)):
            raise ValueError("tied_positions: every sweep must visit each position exactly once")
        if len(blocks) != n_blocks(L, width) or any(len(b) > width or not b for b in blocks):
            raise ValueError(f"tied_positions: a sweep of {L} positions needs {n_blocks(L, width)} blocks of 1..{width} positions")
        nb = len(blocks)
        for b in blocks:
            rows.append(list(b) + [POS_IDLE] * (width - len(b)))
    if nb is None:
        return np.zeros((0, width), dtype=np.int32), 1
    return np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(-1, width)), nb


def tied_rows(n_captions: int, width: int, image_of_caption: Optional[Sequence[int]] = None):
    """Rows of `n_captions` captions polished by `width` slots each: row caption * width + slot.  Returns (groups int32 [R]:
    the caption's index, a valid group id since it is < R; caption_of_row int32 [R]; image_of_row int32 [R]:
    image_of_caption[caption], None = caption c is of image c)."""
    if n_captions < 1 or width < 1:
        raise ValueError("tied_rows: need n_captions >= 1 and width >= 1")
    cap = np.repeat(np.arange(n_captions, dtype=np.int32), width)
    img = cap.copy() if image_of_caption is None else np.asarray(image_of_caption, dtype=np.int32).reshape(-1)[cap]
    if image_of_caption is not None and len(image_of_caption) != n_captions:
        raise ValueError(f"tied_rows: image_of_caption has {len(image_of_caption)} entries for {n_captions} captions")
    return cap.copy(), cap, np.ascontiguousarray(img)


def caption_positions(per_caption: Sequence[np.ndarray]) -> np.ndarray:
    """[n_steps, n_captions * width] from every caption's tied_positions array, in tied_rows' row order."""
    return np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in per_caption], axis=1))


def shuffle_sweeps(L: int, n_sweeps: int, rng) -> Tuple[List[int], List[List[int]]]:
    """The shuffle order as the serial path draws it (gen_utils.py:110-111: ONE `shuffle` of range(L) per call, the same list
    every sweep) -> (order_list, that list once per sweep)."""
    order_list = list(range(L))
    rng.shuffle(order_list)
    return order_list, [list(order_list) for _ in range(n_sweeps)]
