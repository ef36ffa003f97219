"""The fp64 reference of the shared-prefix attention plans (tests/attn_ref.py) against the plain statement it abbreviates,
and the proof that the leak test of tests/test_attention_plan_gpu.py can fail.  CPU only."""
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
