"""The fp64 reference of the shared-prefix attention plans (tests/attn_ref.py) against the plain statement it abbreviates,
and the proof that the leak test of tests/test_attention_plan_gpu.py can fail; the same for the plain segments of
tests/test_attention_seq_gpu.py (seg_ref, its "next" / "prev" / "dup_last" mutants and the inputs on which they show).  CPU only."""
import numpy as np
import pytest

import attn_ref as R


def _random_plan(rng, B, K, max_trunk, max_own, zeros=True):
    trunk = rng.integers(0, max_trunk + 1, size=B)
    own = rng.integers(1, max_own + 1, size=(B, K))
    if zeros:
        own[rng.random((B, K)) < 0.15] = 0
    return trunk, own


@pytest.mark.parametrize("seed", range(6))
def test_plan_reference_equals_the_per_sequence_formula(seed):
    """every candidate's full sequence (trunk rows + own rows) through the per-sequence causal formula in fp64: the plan
    reference must give the same context on every trunk row and every own row, to 1e-12"""
    rng = np.random.default_rng(100 + seed)
    B, K, heads = [(1, 1, 2), (3, 7, 4), (2, 33, 2), (3, 5, 12), (1, 200, 4), (4, 9, 8)][seed]
    trunk, own = _random_plan(rng, B, K, [0, 5, 40, 64, 12, 33][seed], [3, 8, 32, 13, 2, 44][seed])
    if seed == 2:
        trunk[0] = 0
    rows = R.plan_layout(trunk, own)[2]
    qkv = rng.standard_normal((rows, 3 * heads * 64))
    ref = R.plan_ref(qkv, trunk, own, heads, 0.125)
    seqs, lens, src = R.materialise(qkv, trunk, own)
    full = R.seq_ref(seqs, lens, heads, True, 0.125, dtype=np.float64)
    assert full.dtype == np.float64
    # a trunk row appears in its own sequence and in every candidate's: all copies must agree with the plan's one row
    assert np.abs(full - ref[src]).max() < 1e-12
    covered = np.zeros(rows, bool)
    covered[src] = True
    assert covered.all()


def test_rounding_helpers():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 16.0, 65504.0], np.float32)
    assert R.bf16_round(a).tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -6, 16.0]   # ties to even
    assert R.round_operand(R.FP16, a).tolist()[3:] == [16.0, 65504.0]
    assert R.round_operand(R.SPLIT, a) is not None and np.array_equal(R.round_operand(R.SPLIT, a), a)


LEAK_PLAN = (np.array([20, 9, 0]), None)


@pytest.mark.parametrize("kind", ["next", "future", "other"])
@pytest.mark.parametrize("prec", [R.F32, R.BF16, R.FP16, R.SPLIT])
def test_leak_construction_catches_a_mask_widened_by_one_key(kind, prec):
    """(b) of test_attention_plan_gpu.py on the CPU: the bait never reaches the true reference (its outputs stay O(1)),
    while a reference whose mask is wider by ONE key misses the tolerance of that test by >= 50x, in every precision."""
    rng = np.random.default_rng(7)
    B, K, heads = 3, 8, 4
    trunk = np.array([20, 9, 0])
    own = rng.integers(1, 5, size=(B, K))
    own[:, 0] = 4
    rows = R.plan_layout(trunk, own)[2]
    x = R.bait(R.draw_qkv(rng, rows, heads, R.V_SIGMA), trunk, own, kind)
    xr = R.round_operand(prec, x.reshape(rows, -1))
    ref = R.plan_ref(xr, trunk, own, heads, 0.125)
    assert np.abs(ref).max() < 4 * R.V_SIGMA
    tol, merr = R.rounding_tol(prec, xr, trunk, own, heads, 0.125, ref)
    if prec in (R.BF16, R.FP16):
        assert tol <= 2 * R.NORMAL_TOL[prec], (tol, merr)
    wrong = R.plan_ref(xr, trunk, own, heads, 0.125, mutant=kind)
    moved = np.abs(wrong - ref).max()
    print(f"leak {kind:6s} {R.PREC_NAME[prec]:10s}: model error {merr:.2e} tol {tol:.2e}, one leaked key moves the output by {moved:.2f} "
          f"= {moved / tol:.0f} x tol")
    assert moved >= 50 * tol, (moved, tol)


def test_spotlight_construction_puts_the_weight_on_the_target():
    rng = np.random.default_rng(8)
    B, K, heads = 2, 6, 4
    trunk = np.array([33, 0])
    own = rng.integers(1, 6, size=(B, K))
    rows = R.plan_layout(trunk, own)[2]
    for kind in R.SPOT_KINDS:
        x, tgt, trow = R.spotlight(R.draw_qkv(rng, rows, heads, R.V_SIGMA), trunk, own, kind)
        ref, w = R.plan_ref(x.reshape(rows, -1), trunk, own, heads, 0.125, want_weight=tgt)
        assert w.min() > 0.99, (kind, w.min())
        assert np.abs(ref - x[trow, 2].reshape(rows, -1)).max() < 0.05


# ---- plain segments (seg_ref): tests/test_attention_seq_gpu.py ------------------------------------------------------------------
SEG_LENS = [1, 2, 31, 32, 33, 50, 64, 65, 77, 95, 96, 7, 1, 16]
SEG_HEADS, SEG_SCALE = 4, 0.125
SEG_SEEDS = (11, 12)
PRECS = [R.F32, R.BF16, R.FP16, R.SPLIT]
# how many tolerances a reference that is wrong by one key must be away, per precision (the tolerance of f32 / split-fp16 is
# their floor, 2e-5 / 3e-5, so the same move counts for more of them)
LEAK_MOVES = {R.BF16: 20, R.FP16: 200, R.F32: 10000, R.SPLIT: 10000}
DUP_MOVES = {R.BF16: 5, R.FP16: 40, R.F32: 3000, R.SPLIT: 3000}


def _seg_draw(seed, v_sigma=R.V_SIGMA, lens=SEG_LENS):
    return R.draw_qkv(np.random.default_rng(seed), int(np.sum(lens)), SEG_HEADS, v_sigma)


def _seg_tol(prec, xr, causal, ref):
    tol, merr = R.seg_rounding_tol(prec, xr, SEG_LENS, SEG_HEADS, causal, SEG_SCALE, ref)
    if prec in (R.BF16, R.FP16):   # beyond twice the standard-normal bound the construction would be too extreme
        assert tol <= 2 * R.NORMAL_TOL[prec], (tol, merr)
    return tol


@pytest.mark.parametrize("causal", [0, 1])
def test_segment_reference_equals_the_per_sequence_formula(causal):
    lens = SEG_LENS + [0, 5, 0]
    rng = np.random.default_rng(21 + causal)
    qkv = rng.standard_normal((int(np.sum(lens)), 3 * SEG_HEADS * 64))
    ref = R.seg_ref(qkv, lens, SEG_HEADS, causal, SEG_SCALE)
    assert ref.dtype == np.float64
    assert np.abs(ref - R.seq_ref(qkv, lens, SEG_HEADS, bool(causal), SEG_SCALE, dtype=np.float64)).max() < 1e-12
    if causal:   # a plan without trunks and with one candidate per image is a list of causal segments
        plan = R.plan_ref(qkv, np.zeros(len(lens), np.int64), np.asarray(lens)[:, None], SEG_HEADS, SEG_SCALE)
        assert np.abs(ref - plan).max() < 1e-12


def test_segment_reference_weights_and_mutants_are_what_they_say():
    """the weights sum to one over a segment's keys, and each mutant is the plain formula on a sequence with that one key added"""
    lens = [3, 1, 4]
    rng = np.random.default_rng(5)
    qkv = rng.standard_normal((8, 3 * 2 * 64))
    for causal in (0, 1):
        _, pos, ln = R.seg_rows(lens)
        total = sum(R.seg_ref(qkv, lens, 2, causal, 0.125, want_weight=np.minimum(j, ln - 1))[1] * (j < ln)[:, None] for j in range(4))
        assert np.abs(total - 1.0).max() < 1e-12
        pair = R.seg_ref(qkv, lens, 2, causal, 0.125, want_weight=np.stack([pos * 0, pos * 0], 1))[1]
        assert np.abs(pair - R.seg_ref(qkv, lens, 2, causal, 0.125, want_weight=pos * 0)[1]).max() == 0.0
    # bidirectional: segment 1 (row 3) with "next" = rows 3, 4 as one sequence, query 3; with "prev" = rows 2, 3; "dup_last" on
    # segment 0 = rows 0, 1, 2, 2
    full = lambda rows_: R.seq_ref(qkv[rows_], [len(rows_)], 2, False, 0.125, dtype=np.float64)
    assert np.abs(R.seg_ref(qkv, lens, 2, 0, 0.125, mutant="next")[3] - full([3, 4])[0]).max() < 1e-12
    assert np.abs(R.seg_ref(qkv, lens, 2, 0, 0.125, mutant="prev")[3] - full([2, 3])[1]).max() < 1e-12
    assert np.abs(R.seg_ref(qkv, lens, 2, 0, 0.125, mutant="dup_last")[:3] - full([0, 1, 2, 2])[:3]).max() < 1e-12
    assert np.abs(R.seg_ref(qkv, lens, 2, 0, 0.125, mutant="next")[4:] - R.seg_ref(qkv, lens, 2, 0, 0.125)[4:]).max() < 1e-12
    assert np.abs(R.seg_ref(qkv, lens, 2, 0, 0.125, mutant="prev")[:3] - R.seg_ref(qkv, lens, 2, 0, 0.125)[:3]).max() < 1e-12
    # causal "dup_last": query 1 of segment 0 counts key 1 twice
    assert np.abs(R.seg_ref(qkv, lens, 2, 1, 0.125, mutant="dup_last")[1] - full([0, 1, 1])[1]).max() < 1e-12


@pytest.mark.parametrize("seed", SEG_SEEDS)
@pytest.mark.parametrize("prec", PRECS)
def test_segment_leak_construction_catches_a_neighbouring_key(prec, seed):
    """(b) of test_attention_seq_gpu.py on the CPU, both parities and both mask modes: the bait never reaches the true
    reference (it stays O(1)); a reference that also sees the first row after, or the last row before, a victim segment moves
    EVERY victim row that has such a neighbour by >= 20 (bf16), 200 (fp16), 10000 (f32, split-fp16) tolerances."""
    for parity in (0, 1):
        x = R.seg_bait(_seg_draw(seed), SEG_LENS, parity)
        xr = R.round_operand(prec, x.reshape(x.shape[0], -1))
        for causal in (0, 1):
            ref = R.seg_ref(xr, SEG_LENS, SEG_HEADS, causal, SEG_SCALE)
            assert np.abs(ref).max() < 4 * R.V_SIGMA
            tol = _seg_tol(prec, xr, causal, ref)
            for mutant in ("next", "prev"):
                victims = R.seg_victims(SEG_LENS, parity, mutant)
                assert victims.any()
                moved = np.abs(R.seg_ref(xr, SEG_LENS, SEG_HEADS, causal, SEG_SCALE, mutant=mutant) - ref).max(1)[victims]
                print(f"seg leak {mutant} parity {parity} causal {causal} {R.PREC_NAME[prec]:10s}: tol {tol:.2e}, victim rows move by "
                      f"{moved.min() / tol:.0f}..{moved.max() / tol:.0f} x tol")
                assert moved.min() >= LEAK_MOVES[prec] * tol, (mutant, parity, causal, moved.min(), tol)


@pytest.mark.parametrize("seed", SEG_SEEDS)
@pytest.mark.parametrize("prec", PRECS)
def test_segment_spotlights_put_the_weight_on_the_target(prec, seed):
    for causal in (0, 1):
        for kind in R.SEG_SPOT_KINDS:
            x, tgt, trow = R.seg_spotlight(_seg_draw(seed), SEG_LENS, kind, causal)
            xr = R.round_operand(prec, x.reshape(x.shape[0], -1))
            ref, w = R.seg_ref(xr, SEG_LENS, SEG_HEADS, causal, SEG_SCALE, want_weight=tgt)
            assert w.min() > 0.99, (kind, causal, w.min())
            assert np.abs(ref - xr.reshape(-1, 3, SEG_HEADS * 64)[trow, 2]).max() < 0.05
            _seg_tol(prec, xr, causal, ref)
    _, pos, ln = R.seg_rows(SEG_LENS)
    assert {int(t) for t in R.seg_spotlight(_seg_draw(seed), SEG_LENS, "key64", 0)[1]} == {int(min(64, n - 1)) for n in SEG_LENS}


@pytest.mark.parametrize("seed", SEG_SEEDS)
@pytest.mark.parametrize("prec", PRECS)
def test_segment_twin_construction_catches_a_last_key_counted_twice(prec, seed):
    """(c) of test_attention_seq_gpu.py on the CPU: key 0 and the last visible key share > 0.99 of the weight, and a reference
    that counts the last visible key twice moves EVERY row whose two targets differ by >= 5 (bf16), 40 (fp16), 3000 (f32,
    split-fp16) tolerances."""
    for causal in (0, 1):
        x, pair = R.seg_twin(_seg_draw(seed), SEG_LENS, causal)
        xr = R.round_operand(prec, x.reshape(x.shape[0], -1))
        ref, w = R.seg_ref(xr, SEG_LENS, SEG_HEADS, causal, SEG_SCALE, want_weight=pair)
        assert w.min() > 0.99, (causal, w.min())
        tol = _seg_tol(prec, xr, causal, ref)
        differ = pair[:, 0] != pair[:, 1]
        assert differ.any() and not differ.all()
        moved = np.abs(R.seg_ref(xr, SEG_LENS, SEG_HEADS, causal, SEG_SCALE, mutant="dup_last") - ref).max(1)
        print(f"seg twin causal {causal} {R.PREC_NAME[prec]:10s}: tol {tol:.2e}, pair weight >= {w.min():.4f}, a doubled last key moves "
              f"the rows by {moved[differ].min() / tol:.1f}..{moved[differ].max() / tol:.1f} x tol")
        assert moved[differ].min() >= DUP_MOVES[prec] * tol, (causal, moved[differ].min(), tol)
