"""The integer kernels of csrc/rowops.hip (row gathers, masks, tied rows), csrc/memo.hip and csrc/memo_rows.hip, one launcher chain at
a time, against the numpy models of tests/memo_ref.py, word for word on WHOLE buffers (what a kernel must not write is compared too:
it holds its input, or the hooks' pre-fill pattern) and with guard words around every output.  The memo checks run at batch sizes on both
sides of their 256-row chunks, which no whole-step test reaches."""
import numpy as np
import pytest

import kernel_hooks as KH
import memo_ref as MR

pytestmark = pytest.mark.gpu


def _same(g, model, names=None):
    g.assert_guards()
    for name in names or g.keys():
        assert MR.same_words(g[name], model[name]), (name, np.nonzero(np.asarray(g[name]).reshape(-1).view(np.uint32)
                                                                     != np.ascontiguousarray(model[name]).reshape(-1).view(np.uint32))[0][:8])


def _untouched(g):
    g.assert_guards()
    return all(KH.untouched(v).all() for v in g.values())


# ---- movers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,widths", [(0, (4, 256, 260, 1028)), (1, (16, 128, 1040, 2048)), (2, (1, 2, 3, 77))])
def test_gather_rows(kind, widths):
    """launch_gather_rows_f32 (W floats) / _bytes (W bytes) / _w32 (W words): dst[m] = src[idx[m]] bit for bit, repeats in idx, one
    row, a full and a partial work-group of four rows, many work-groups; widths around the 256-float / 1024-byte stride of a wave"""
    rng = np.random.default_rng(kind)
    for W in widths:
        rw = W // 4 if kind == 1 else W
        src = rng.integers(0, 2 ** 32, (40, rw), dtype=np.uint64).astype(np.uint32)
        src[src == KH.SENTINEL] = 1
        for M in (1, 4, 5, 300):
            idx = rng.integers(0, 40, M).astype(np.int32)
            if M > 1:
                idx[1] = idx[0]
            ref, out = KH.gather_rows(kind, src, idx, W)
            assert not ref
            _same(out, {"dst": MR.gather_rows(src, idx)})


def test_gather_launchers_refuse_rows_that_are_not_whole_vectors():
    src = np.ones((8, 6), np.uint32)
    idx = np.array([3, 3, 0, 7, 1], np.int32)
    for kind, W in ((0, 6), (0, 2), (1, 24), (1, 8)):
        ref, out = KH.gather_rows(kind, src[:, :W // 4 if kind == 1 else W], idx, W)
        assert ref and _untouched(out)


def test_mask_positions():
    rng = np.random.default_rng(5)
    B, T = 150, 12   # B * n_mask = 300 threads: more than one work-group
    inp = rng.integers(5, 1000, (B, T)).astype(np.int32)
    for n_mask in (0, 1, 2):
        for gen in (0, 4, T - 1):   # the window at T - 1 runs past the row and is clipped
            ref, out = KH.mask_positions(inp, gen, n_mask, MR.MASK_ID)
            assert not ref
            _same(out, {"inp": MR.mask_positions(inp, gen, n_mask, MR.MASK_ID)})
        gen = rng.integers(0, T, B).astype(np.int32)
        gen[3::11] = T - 1
        gen[::7] = -1        # the row is left alone
        ref, out = KH.mask_positions(inp, gen, n_mask, MR.MASK_ID)
        assert not ref
        _same(out, {"inp": MR.mask_positions(inp, gen, n_mask, MR.MASK_ID)})
        assert np.array_equal(out["inp"].reshape(B, T)[::7], inp[::7])


def test_tie_rows():
    """R = 300 rows in CSR groups of 1, 2 and 5 (members scattered over the batch), columns that include idle rows and a column >= T;
    the members of a group run at distinct columns (the host's guarantee, asserted here on the inputs)."""
    rng = np.random.default_rng(6)
    R, T = 300, 8
    inp = rng.integers(5, 1000, (R, T)).astype(np.int32)
    order = rng.permutation(R)
    sizes = []
    while sum(sizes) < R:
        sizes.append(min((1, 2, 5)[len(sizes) % 3], R - sum(sizes)))
    grp_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    grp_rows = order.astype(np.int32)
    grp_of_row = np.empty(R, np.int32)
    col = np.empty(R, np.int32)
    for g, n in enumerate(sizes):
        members = grp_rows[grp_off[g]:grp_off[g + 1]]
        grp_of_row[members] = g
        cols = list(rng.permutation(T)[:n])
        if n == 5:
            cols[3], cols[4] = MR.POS_IDLE, T + 1
        col[members] = cols
    assert MR.tie_inputs_ok(col, grp_off, grp_rows, T) and {1, 2, 5} <= set(sizes)
    ref, out = KH.tie_rows(inp, col, grp_of_row, grp_off, grp_rows)
    assert not ref
    exp = MR.tie_rows(inp, col, grp_of_row, grp_off, grp_rows)
    assert (exp != inp).any()
    _same(out, {"inp": exp})


# ---- image memo -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 255, 256, 257, 700])
def test_memo_check(B):
    """memo_check_kernel walks the batch in chunks of 256 with a running base: hit, the ascending list of the others (entries behind it
    keep the pattern), tot = (count, max of img_max over the hit images per sub-step, 0)"""
    T, D = 12, 4
    for pattern in MR.MEMO_PATTERNS:
        for n_mask, gen_idx in ((0, 4), (1, 4), (2, 4), (2, T - 1)):
            for n_sub in (1, 2):
                st = MR.memo_state(B, T, D, gen_idx, n_mask, pattern)
                ref, out = KH.memo_chain(st, gen_idx, n_mask, MR.MASK_ID, n_sub, stages=0)
                assert not ref
                model = MR.memo_chain(st, gen_idx, n_mask, MR.MASK_ID, n_sub, stages=0)
                n = int(model["tot"][0])
                assert n == int(st["miss"].sum()) and model["tot"][3] == 0 and (np.diff(model["list"][:n]) > 0).all()
                _same(out, model)


@pytest.mark.parametrize("B", [64, 257, 700])
def test_memo_chain(B):
    """check -> fill -> gather -> (the step: host-given rows, cosines, longest branches) -> scatter, with and without a list, recording
    or not: every buffer against the model, so the keys, entries and rows of images not listed are seen unchanged"""
    T, D, gen_idx = 12, 8, 4
    for pattern in ("alternating", "chunk_last", "random", "all_hit", "all_miss"):
        for n_mask in (1, 2):
            st = MR.memo_state(B, T, D, gen_idx, n_mask, pattern)
            for use_list in (0, 1):
                for record in (0, 1):
                    ref, out = KH.memo_chain(st, gen_idx, n_mask, MR.MASK_ID, 2, 1, use_list, record)
                    assert not ref
                    _same(out, MR.memo_chain(st, gen_idx, n_mask, MR.MASK_ID, 2, 1, use_list, record))


# ---- rows memo ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 63, 64, 65, 255, 256, 257, 600])
def test_memo_rows_check(R):
    """memo_rows_flag_kernel / memo_rows_list_kernel split the rows over (R + 255) / 256 work-groups and rebuild one ascending list from
    the per-group counts: hit (0 / 1 / 2 = idle), cnt, list, tot -- with idle rows, valid == 0, each signature field differing, col1
    null, drawing rows, columns outside the caption and imax <= 0 in the "mixed" pattern"""
    T, L, seed_len, D = 12, 3, 4, 4
    for pattern in MR.ROWS_PATTERNS:
        for n_mask0, n_sub, with_col1 in ((1, 1, False), (2, 2, True), (0, 2, False), (1, 2, True)):
            st = MR.rows_state(R, T, L, seed_len, D, n_mask0, n_sub, pattern, with_col1)
            ref, out = KH.memo_rows_chain(st, L, seed_len, n_mask0, n_sub, MR.MASK_ID, stages=0)
            assert not ref
            model = MR.rows_chain(st, L, seed_len, n_mask0, n_sub, MR.MASK_ID, stages=0)
            n = int(model["tot"][0])
            assert (np.diff(model["list"][:n]) > 0).all() and model["cnt"].size == (R + 255) // 256
            _same(out, model)


@pytest.mark.parametrize("R", [65, 257, 600])
def test_memo_rows_chain(R):
    T, L, seed_len, D = 12, 3, 4, 8
    for pattern in ("alternating", "chunk_last", "mixed", "all_hit", "all_miss"):
        for n_mask0, n_sub, with_col1 in ((1, 1, False), (2, 2, True)):
            st = MR.rows_state(R, T, L, seed_len, D, n_mask0, n_sub, pattern, with_col1)
            for j in (0, 1):
                for use_list in (0, 1):
                    for record in (0, 1):
                        ref, out = KH.memo_rows_chain(st, L, seed_len, n_mask0, n_sub, MR.MASK_ID, j, 1, use_list, record)
                        assert not ref
                        _same(out, MR.rows_chain(st, L, seed_len, n_mask0, n_sub, MR.MASK_ID, j, 1, use_list, record))
