"""The numpy models of tests/memo_ref.py against what their inputs were built to mean (the state builders know which rows they
perturbed) and against plain loops: the models are the reference of tests/test_mover_memo_kernels_gpu.py, so they get tests of their own."""
import numpy as np
import pytest

import memo_ref as MR


def test_masked_and_mask_positions_against_loops():
    rng = np.random.default_rng(1)
    inp = rng.integers(5, 99, (7, 12)).astype(np.int32)
    gen = np.array([0, 11, 10, -1, 5, 12, 3], np.int32)
    for n_mask in (0, 1, 2, 3):
        exp = inp.copy()
        for b in range(7):
            for j in range(n_mask):
                if gen[b] >= 0 and gen[b] + j < 12:
                    exp[b, gen[b] + j] = 3
        assert np.array_equal(MR.mask_positions(inp, gen, n_mask, 3), exp)
        exp = inp.copy()
        exp[:, 10:10 + n_mask] = 3   # clipped at T
        assert np.array_equal(MR.mask_positions(inp, 10, n_mask, 3), exp)


def test_tie_rows_members_agree_where_one_of_them_ran():
    rng = np.random.default_rng(2)
    inp = rng.integers(5, 99, (8, 6)).astype(np.int32)
    grp_off = np.array([0, 1, 3, 8])
    grp_rows = np.array([0, 2, 5, 1, 3, 4, 6, 7])
    grp_of_row = np.array([0, 2, 1, 2, 2, 1, 2, 2])
    col = np.array([2, 0, 1, MR.POS_IDLE, 3, 4, 9, 5])
    assert MR.tie_inputs_ok(col, grp_off, grp_rows, 6)
    assert not MR.tie_inputs_ok(np.array([2, 0, 1, 0, 3, 4, 9, 5]), grp_off, grp_rows, 6)
    out = MR.tie_rows(inp, col, grp_of_row, grp_off, grp_rows)
    assert np.array_equal(out[0], inp[0])                              # a group of one
    assert out[5, 1] == inp[2, 1] and out[2, 4] == inp[5, 4]          # a pair, both ways
    for m in (1, 3, 4, 6, 7):                                          # the group of five: columns 0, 3, 5 ran; idle and >= T did not
        assert out[m, 0] == inp[1, 0] and out[m, 3] == inp[4, 3] and out[m, 5] == inp[7, 5]
        assert np.array_equal(out[m, [1, 2, 4]], inp[m, [1, 2, 4]])


@pytest.mark.parametrize("B", [1, 64, 257])
@pytest.mark.parametrize("pattern", MR.MEMO_PATTERNS)
def test_memo_chain_model(B, pattern):
    T, D, gen_idx = 12, 8, 4
    for n_mask in (0, 1, 2):
        st = MR.memo_state(B, T, D, gen_idx, n_mask, pattern)
        miss = st["miss"]
        o = MR.memo_chain(st, gen_idx, n_mask, MR.MASK_ID, 2, stages=0)
        n = int(miss.sum())
        assert np.array_equal(o["hit"], (~miss).astype(np.int32)) and o["tot"][0] == n and o["tot"][3] == 0
        assert np.array_equal(o["list"][:n], np.nonzero(miss)[0]) and (o["list"][n:].view(np.uint32) == MR.SENT).all()
        for j in range(2):
            assert o["tot"][1 + j] == max([int(st["img_max"][j, b]) for b in range(B) if not miss[b]], default=0)
        for use_list in (0, 1):
            for record in (0, 1):
                o = MR.memo_chain(st, gen_idx, n_mask, MR.MASK_ID, 2, 1, use_list, record)
                for b in range(B):
                    if not miss[b] and n < B:       # a hit image takes the entry back (unless the whole batch ran in place)
                        if use_list or n == 0:
                            assert np.array_equal(o["inp"][b], st["ent_rows"][b]) and o["bcos"][b] == st["ent_cos"][b]
                    if miss[b]:
                        assert o["bcos"][b] == st["new_cos"][b]
                        assert np.array_equal(o["inp"][b], st["new_rows"][b] if use_list else st["inp"][b])
                        if record:
                            assert np.array_equal(o["key"][b], MR.masked(st["inp"][b:b + 1], gen_idx, n_mask, MR.MASK_ID)[0])
                            assert np.array_equal(o["ent_rows"][b], st["new_rows"][b]) and o["ent_max"][b] == st["new_max"][b]
                    if not record or (use_list and not miss[b]) or n == 0:
                        assert np.array_equal(o["ent_rows"][b], st["ent_rows"][b]) and np.array_equal(o["key"][b], st["key"][b])
                if use_list and n:
                    assert np.array_equal(o["inp_c"][:n], st["inp"][miss]) and MR.same_words(o["img_c"][:n], st["img_n"][miss])
                    assert (o["inp_c"][n:].view(np.uint32) == MR.SENT).all()


@pytest.mark.parametrize("R", [1, 65, 257])
@pytest.mark.parametrize("pattern", MR.ROWS_PATTERNS)
def test_rows_chain_model_against_a_loop(R, pattern):
    T, L, seed_len, D = 12, 3, 4, 8
    for n_mask0, n_sub, with_col1 in ((1, 1, False), (2, 2, True), (0, 2, False)):
        st = MR.rows_state(R, T, L, seed_len, D, n_mask0, n_sub, pattern, with_col1)
        o = MR.rows_chain(st, L, seed_len, n_mask0, n_sub, MR.MASK_ID, stages=0)
        hit, lst, tot = [], [], [0, 0, 0, 0]
        for r in range(R):   # memo_rows_flag_kernel, one row at a time
            c0 = int(st["col0"][r])
            if c0 < 0:
                hit.append(MR.IDLE)
                continue
            p = c0 - seed_len
            same = 0 <= p < L
            if same:
                sg = (n_mask0 & 0xFF) | (n_sub << 8) | ((int(st["col1"][r]) + 1 if n_sub > 1 and st["col1"] is not None else 0) << 16)
                same = st["valid"][p, r] == 1 and st["sig"][p, r] == sg and not (st["tau"] is not None and st["tau"][r] > 0)
                row = [MR.MASK_ID if c0 <= t < c0 + n_mask0 else int(st["inp"][r, t]) for t in range(T)]
                same = same and row == st["key"][p, r].tolist()
            if same:
                for j in range(n_sub):
                    tot[1 + j] = max(tot[1 + j], int(st["imax"][p, j, r]))
            else:
                lst.append(r)
            hit.append(MR.HIT if same else MR.MISS)
        tot[0] = len(lst)
        assert o["hit"].tolist() == hit and o["tot"].tolist() == tot and o["list"][:len(lst)].tolist() == lst
        assert o["cnt"].size == (R + 255) // 256 and int(o["cnt"].sum()) == len(lst)
        if pattern == "mixed" and R > 64:
            assert {MR.MISS, MR.HIT, MR.IDLE} <= set(hit)
        # the chain: listed rows take the step's result, hit rows their slot, idle rows nothing; only the slots of recorded rows change
        o = MR.rows_chain(st, L, seed_len, n_mask0, n_sub, MR.MASK_ID, j=1, stages=1, use_list=1, record=1)
        changed = np.zeros((L, R), bool)
        for r in range(R):
            p = int(st["col0"][r]) - seed_len
            if hit[r] == MR.MISS:
                assert np.array_equal(o["inp"][r], st["new_rows"][r]) and o["bcos"][r] == st["new_cos"][r]
                if 0 <= p < L:
                    changed[p, r] = True
                    assert o["valid"][p, r] == 1 and np.array_equal(o["rows"][p, 1, r], st["new_rows"][r]) and o["imax"][p, 1, r] == st["new_max"][r]
            elif hit[r] == MR.HIT:
                assert np.array_equal(o["inp"][r], st["rows"][p, 1, r]) and o["bcos"][r] == st["cos"][p, 1, r]
            else:
                assert np.array_equal(o["inp"][r], st["inp"][r]) and o["bcos"][r] == st["bcos"][r]
        for name in ("valid", "sig", "key"):
            assert np.array_equal(o[name][~changed], st[name][~changed]), name
        assert np.array_equal(o["rows"][:, 0], st["rows"][:, 0]) and np.array_equal(o["rows"][:, 1][~changed], st["rows"][:, 1][~changed])
