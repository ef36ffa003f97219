"""conzic_amd/blocks.py: the schedules of block-synchronous sweeps (czc_generate_rows_tied).  No GPU, no engine."""
import math
import random

import numpy as np
import pytest

from conzic_amd import blocks as B, harness
from oracle import step as S

IDLE = B.POS_IDLE
SHAPES = [(L, W) for L in (1, 2, 5, 6, 7, 10, 11) for W in (1, 2, 3, 4, 5, 7, 10, 11, 16)]


@pytest.mark.parametrize("L,W", SHAPES)
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_every_position_once_per_sweep(L, W, layout):
    blocks = B.sequential_order(L, W, layout)
    assert len(blocks) == math.ceil(L / W)
    assert sorted(p for b in blocks for p in b) == list(range(L))
    assert all(1 <= len(b) <= W for b in blocks)
    pos, every = B.tied_positions([blocks] * 3, W)
    assert every == len(blocks) and pos.shape == (3 * every, W) and pos.dtype == np.int32
    for s in range(3):
        sweep = pos[s * every:(s + 1) * every]
        assert sorted(int(p) for p in sweep.ravel() if p != IDLE) == list(range(L))


@pytest.mark.parametrize("L,W", SHAPES)
def test_interleaved_blocks_hold_no_neighbours(L, W):
    blocks = B.sequential_order(L, W, "interleaved")
    nb = len(blocks)
    for i, b in enumerate(blocks):
        assert b == list(range(i, L, nb))          # i, i + nb, i + 2 nb, ...
        if nb >= 2:
            assert all(abs(p - q) != 1 for p in b for q in b)
    sizes = [len(b) for b in blocks]
    assert sizes == sorted(sizes, reverse=True) and sizes[0] - sizes[-1] <= 1


@pytest.mark.parametrize("L", [2, 5, 6, 10, 11])
def test_half_width_is_red_black(L):
    blocks = B.sequential_order(L, math.ceil(L / 2), "interleaved")
    assert blocks == [list(range(0, L, 2)), list(range(1, L, 2))]


@pytest.mark.parametrize("L,W", [(5, 5), (5, 8), (1, 1), (10, 10), (10, 64)])
@pytest.mark.parametrize("layout", B.LAYOUTS)
def test_width_of_the_sentence_is_one_block(L, W, layout):
    assert B.sequential_order(L, W, layout) == [list(range(L))]
    pos, every = B.tied_positions([B.sequential_order(L, W, layout)] * 2, W)
    assert every == 1 and pos.shape[0] == 2


@pytest.mark.parametrize("L,W", SHAPES)
def test_idle_slots_only_in_a_short_last_block(L, W):
    """Consecutive blocks (the contiguous layout, a shuffled order): every block but the last is full.  The interleaved
    layout deals round-robin, so its short blocks are the trailing ones (checked above); idle slots are a block's tail."""
    order = S.shuffle_order(L, seed=L * 31 + W)
    for sweep in (B.sequential_order(L, W, "contiguous"), order):
        pos, nb = B.tied_positions([sweep], W)
        assert (pos[:-1] != IDLE).all()
        assert (pos[-1] != IDLE).sum() == L - (nb - 1) * W
    pos, nb = B.tied_positions([B.sequential_order(L, W, "interleaved")], W)
    for row in pos:
        n = int((row != IDLE).sum())
        assert n >= 1 and (row[:n] != IDLE).all() and (row[n:] == IDLE).all()
    assert int((pos == IDLE).sum()) == nb * W - L


def test_contiguous_layout():
    assert B.sequential_order(10, 4, "contiguous") == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert B.sequential_order(10, 4, "interleaved") == [[0, 3, 6, 9], [1, 4, 7], [2, 5, 8]]
    with pytest.raises(ValueError):
        B.sequential_order(10, 4, "diagonal")
    with pytest.raises(ValueError):
        B.sequential_order(10, 0)


@pytest.mark.parametrize("L,W", [(6, 3), (10, 4), (7, 7)])
def test_shuffle_consumes_the_rng_as_run_generation_does(L, W):
    """One shuffle of range(L) per call, the same list every sweep (gen_utils.py:110-111); afterwards the stream stands where
    the serial path leaves it."""
    a, b = random.Random(1234), random.Random(1234)
    want = S.shuffle_order(L, rng=a)
    order_list, sweeps = B.shuffle_sweeps(L, 3, b)
    assert order_list == want and sweeps == [want] * 3
    assert a.random() == b.random()
    pos, nb = B.tied_positions(sweeps, W)
    for s in range(3):
        got = [int(p) for p in pos[s * nb:(s + 1) * nb].ravel() if p != IDLE]
        assert got == want            # consecutive blocks of the drawn permutation
    assert B.block_schedule(want, W) == [want[i:i + W] for i in range(0, L, W)]


@pytest.mark.parametrize("L,W,layout", [(6, 3, "interleaved"), (10, 4, "contiguous"), (5, 2, "interleaved"), (6, 6, "interleaved")])
def test_tied_rows_put_no_two_slots_of_a_group_on_one_column(L, W, layout):
    n_cap = 3
    groups, cap, ior = B.tied_rows(n_cap, W, image_of_caption=[0, 1, 0])
    assert groups.tolist() == cap.tolist() == [c for c in range(n_cap) for _ in range(W)]
    assert ior.tolist() == [[0, 1, 0][c] for c in cap]
    assert (groups >= 0).all() and (groups < n_cap * W).all()
    one, nb = B.tied_positions([B.sequential_order(L, W, layout)] * 2, W)
    pos = B.caption_positions([one] * n_cap)
    assert pos.shape == (2 * nb, n_cap * W)
    for s in range(pos.shape[0]):
        for g in range(n_cap):
            cols = [int(p) for p in pos[s, groups == g] if p != IDLE]
            assert len(cols) == len(set(cols)) >= 1
    assert B.tied_rows(2, 3)[2].tolist() == [0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("order", ["sequential", "shuffle"])
def test_width_one_is_the_untied_schedule(order):
    L, iters = 6, 3
    order_list = S.shuffle_order(L, seed=3) if order == "shuffle" else None
    want, n_mask, every = harness.order_positions(order, L, iters, order_list=order_list)
    sweeps = [order_list] * iters if order == "shuffle" else [B.sequential_order(L, 1, "interleaved")] * iters
    pos, nb = B.tied_positions(sweeps, 1)
    assert nb == every == L and pos[:, 0].tolist() == want and set(n_mask) == {1}
    assert B.sequential_order(L, 1, "contiguous") == B.sequential_order(L, 1, "interleaved") == [[p] for p in range(L)]


def test_resolve_width():
    assert B.resolve_width(0, 10) == 10 and B.resolve_width(3, 10) == 3 and B.resolve_width(64, 10) == 10
    with pytest.raises(ValueError):
        B.resolve_width(-1, 10)
    with pytest.raises(ValueError):
        B.tied_positions([[0, 1, 1]], 2)
