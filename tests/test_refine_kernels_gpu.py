"""The kernels between the two text-tower passes of the screen-then-refine engine, one launcher chain at a time, against
tests/refine_ref.py: scan_kernel, prefix_plan_kernel (with exact de-duplication) and prefix_finish_kernel, refine_select_kernel in
its three launch forms and four instantiations (selection, stratified sample, margin gate), refine_plan_kernel and
refine_finish_kernel, refine_cosine_kernel and the refine_kind branch of combine_kernel.

The hooks (tests/kernel_hooks.py: scan .. combine_refine) run the launchers in the engine's order with the engine's buffer
preparation; every output sits inside a larger allocation pre-filled with a byte pattern, so each test also asserts that the
guard words around an output are intact and that the words a kernel is documented not to write still hold the pattern.

Integer outputs and the selection are compared exactly (the conditions that makes legitimate -- no clip_score within 4 ulp of its
threshold -- are asserted by the reference on every call and, for these inputs, in tests/test_refine_ref_cpu.py).  The margin
gate is held to the float64 reference outside a band of 32 eps max(1, beta): it must not pass a row whose winner the adversarial
errors overturn by more than the band and must pass a row that is safe by more than the band.  Cosines and scores: float64, the
tolerances of test_kernels_gpu.py::test_fused_score_combine."""
import functools

import numpy as np
import pytest

import kernel_hooks as KH
import refine_ref as R
from conzic_amd import native

pytestmark = pytest.mark.gpu


def eq(got, want, what):
    got, want = np.asarray(got, np.int64).reshape(-1), np.asarray(want, np.int64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {int(bad[0])}: kernel {got[bad[0]]}, reference {want[bad[0]]}"


def eq_or_untouched(got, want, what):
    """want: list whose None entries the kernels must leave alone"""
    keep = np.array([w is None for w in want])
    assert KH.untouched(got)[keep].all(), f"{what}: a word outside the plan was written"
    eq(np.asarray(got)[~keep], [w for w in want if w is not None], what)


def hyper(beta):
    return native.Hyper(0.02, float(beta), 0.0, 0.1, 0, 0)


# ---- scan -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SCAN_N)
def test_scan(n):
    v = R.scan_lengths(n)
    off, tot, mx = R.scan(v)
    res = KH.scan(v)
    res.assert_guards()
    eq(res["off"], off, "off")
    eq(res["totals"], [tot, mx], "totals")


# ---- shared-prefix plan ---------------------------------------------------------------------------------------------------------------
PLAN_TABLES = ("own_len", "pre_len", "seg_src", "seg_pos0", "own_off", "pre_off", "eos_idx", "img_max", "totals")


@pytest.mark.parametrize("K", R.PLAN_K)
@pytest.mark.parametrize("B", R.PLAN_B)
def test_prefix_plan(B, K):
    ids, length = R.plan_rows(B, K)
    for share in (0, 1):
        for dedup in (0, 1):
            ref = R.prefix_plan(ids, length, share, dedup)
            res = KH.prefix_plan(ids, length, share, dedup)
            res.assert_guards()
            for name in PLAN_TABLES:
                eq(res[name], ref[name], f"{name} (share {share}, dedup {dedup})")
            if dedup:
                eq(res["rep"], ref["rep"], f"rep (share {share})")
            else:
                assert KH.untouched(res["rep"]).all()


def test_prefix_plan_dedup_refuses_more_than_1024_candidates():
    """the de-duplication keeps one hash per candidate in LDS: K > 1024 is an error of the launcher, not a launch"""
    rng = np.random.default_rng(1)
    K = 1025
    ids = rng.integers(1000, 40000, size=(1, K, R.CLIP_LEN)).astype(np.int32)
    length = rng.integers(2, R.CLIP_LEN + 1, size=(1, K)).astype(np.int32)
    with pytest.raises(native.NativeError, match="de-duplication needs K <= 1024"):
        KH.prefix_plan(ids, length, 1, 1)
    ref = R.prefix_plan(ids, length, 1, 0)      # without it the plan serves any K
    res = KH.prefix_plan(ids, length, 1, 0)
    res.assert_guards()
    for name in PLAN_TABLES:
        eq(res[name], ref[name], name)


# ---- selection and margin gate ------------------------------------------------------------------------------------------------------------
def check_select(res, p, f, thetas, betas, taus, h, m, need_cos, planted=False):
    """One launch of any form against the reference, row by row.  A row the kernel gated is recognised by what a full selection
    never leaves: no kind-1 candidate (its winner always is one)."""
    B, K = p.shape
    res.assert_guards()
    n_gated = n_elig = 0
    for b in range(B):
        kind, lst, count = res["kind"][b], res["list"][b], int(res["count"][b])
        assert not KH.untouched(kind).any(), (b, "kind not written")
        gated = not ((kind & 3) == 1).any()
        if h <= 0 or taus[b] > 0:
            assert not gated, (b, "a row that draws, or a launch without the gate, was gated")
        else:
            n_elig += 1
            v = R.gate_verdict(p[b], f[b], betas[b], h)
            assert not (v == 1 and not gated), (b, "the gate refused a row that is safe by more than the band",
                                                R.gate_worst64(p[b], f[b], betas[b], h))
            assert not (v == -1 and gated), (b, "the gate passed a row whose winner can be overturned",
                                             R.gate_worst64(p[b], f[b], betas[b], h))
        if gated:
            n_gated += 1
            want = R.gated_row(K, R.first_argmax(f[b]), need_cos)
        else:
            want = R.select_row(p[b], f[b], thetas[b], m, planted=planted)
            R.check_selection_properties(kind, p[b], thetas[b], m, lst, count)
        eq(kind, want, f"kind of row {b}")
        nz = np.nonzero(want)[0]
        assert count == nz.size, (b, count, nz.size)
        eq(lst[:count], nz, f"list of row {b}")
        assert KH.untouched(lst[count:]).all(), (b, "list written behind count")
    eq(res["gated"], [n_gated, n_elig], "gated")
    return n_gated


@pytest.mark.parametrize("K", R.SEL_K)
def test_refine_select(K):
    p, f = R.sel_inputs(K)
    B = R.SEL_B
    th = R.sel_theta(K)
    zeros = [0.0] * B
    row_thetas = [R.theta_of_row(R.SEL_THETA_BASE, R.SEL_SCALE, b) for b in R.SEL_BETAS]
    hps = [hyper(b) for b in R.SEL_BETAS]
    draws = [native.Draw(17 + b, float(t), 0) for b, t in enumerate(R.SEL_TAUS)]
    for m in R.sel_m_samples(K):
        # form 0: one threshold for the launch
        check_select(KH.refine_select(0, p, f, m, 0.0, 0, theta=th, beta=1.0), p, f, [th] * B, [1.0] * B, zeros, 0.0, m, 0)
        # form 1 and both instantiations of form 2: the row's own beta and threshold; rows 1 and 4 draw
        check_select(KH.refine_select(1, p, f, m, 0.0, 1, theta_base=R.SEL_THETA_BASE, scale=R.SEL_SCALE, hyper=hps),
                     p, f, row_thetas, R.SEL_BETAS, zeros, 0.0, m, 1)
        check_select(KH.refine_select(2, p, f, m, 0.0, 1, theta_base=R.SEL_THETA_BASE, scale=R.SEL_SCALE, hyper=hps, draws=draws),
                     p, f, row_thetas, R.SEL_BETAS, R.SEL_TAUS, 0.0, m, 1)
        check_select(KH.refine_select(2, p, f, m, 0.0, 0, theta=th, beta=1.0, draws=draws), p, f, [th] * B, [1.0] * B, R.SEL_TAUS, 0.0, m, 0)
    # a clip_score EQUAL to the threshold is not above it
    pp, _ = R.sel_inputs(K, planted=True)
    check_select(KH.refine_select(0, pp, f, 24, 0.0, 0, theta=th, beta=1.0), pp, f, [th] * B, [1.0] * B, zeros, 0.0, 24, 0, planted=True)


@pytest.mark.parametrize("K", R.SEL_K)
def test_refine_select_scalar_and_uniform_rows_agree(K):
    p, f = R.sel_inputs(K)
    for beta in (2.0, 0.5):
        th = R.theta_of_row(R.SEL_THETA_BASE, R.SEL_SCALE, beta)
        h = R.GATE_DELTA * R.SEL_SCALE
        a = KH.refine_select(0, p, f, 24, h, 1, theta=th, beta=beta)
        b = KH.refine_select(1, p, f, 24, h, 1, theta_base=R.SEL_THETA_BASE, scale=R.SEL_SCALE, hyper=[hyper(beta)] * R.SEL_B)
        for name in ("gated", "kind", "list", "count"):
            assert np.array_equal(a[name], b[name]), name


@functools.lru_cache(maxsize=None)
def gate_case(K, scale, beta):
    return R.gate_inputs(K, scale, beta)


GATE_LOG = {"rows": 0, "gated": 0}


@pytest.mark.parametrize("K,scale,beta,need_cos", R.gate_cases())
def test_margin_gate(K, scale, beta, need_cos):
    p, f, h = gate_case(K, scale, beta)
    B = R.GATE_B
    theta = R.theta_of_row(R.SEL_THETA_BASE, scale, beta)
    zeros = [0.0] * B
    taus = [0.5 if b % 4 == 1 else 0.0 for b in range(B)]
    draws = [native.Draw(5 + b, t, 0) for b, t in enumerate(taus)]
    hps = [hyper(beta)] * B
    n = check_select(KH.refine_select(0, p, f, 12, h, need_cos, theta=theta, beta=beta), p, f, [theta] * B, [beta] * B, zeros, h, 12, need_cos)
    GATE_LOG["rows"] += B
    GATE_LOG["gated"] += n
    print(f"gate K={K} scale={scale} beta={beta}: {n}/{B} rows gated ({GATE_LOG['gated']}/{GATE_LOG['rows']} so far)")
    check_select(KH.refine_select(1, p, f, 12, h, need_cos, theta_base=R.SEL_THETA_BASE, scale=scale, hyper=hps),
                 p, f, [theta] * B, [beta] * B, zeros, h, 12, need_cos)
    # rows that draw are never gated nor counted, with either source of beta
    check_select(KH.refine_select(2, p, f, 12, h, need_cos, theta=theta, beta=beta, draws=draws), p, f, [theta] * B, [beta] * B, taus, h, 12, need_cos)
    # ... and with a beta of its own per row: the gate and the threshold take the row's
    betas = R.gate_row_betas(beta)
    thetas = [R.theta_of_row(R.SEL_THETA_BASE, scale, bt) for bt in betas]
    check_select(KH.refine_select(2, p, f, 12, h, need_cos, theta_base=R.SEL_THETA_BASE, scale=scale, hyper=[hyper(bt) for bt in betas],
                                  draws=draws), p, f, thetas, betas, taus, h, 12, need_cos)
    check_select(KH.refine_select(1, p, f, 12, h, need_cos, theta_base=R.SEL_THETA_BASE, scale=scale, hyper=[hyper(bt) for bt in betas]),
                 p, f, thetas, betas, zeros, h, 12, need_cos)


def test_margin_gate_never_passes_a_nan_score():
    K, scale, beta = 200, 100.0, 1.0
    p, f, h = gate_case(K, scale, beta)
    safe = [b for b in range(R.GATE_B) if R.gate_verdict(p[b], f[b], beta, h) == 1][:4]
    assert len(safe) == 4
    f = f.copy()
    for i, b in enumerate(safe[:3]):            # a challenger in the first, a later and the last pass of the 256-thread loop
        w = R.first_argmax(f[b])
        k = (3, 150, K - 1)[i]
        f[b, k if k != w else k - 1] = np.nan
    theta = R.theta_of_row(R.SEL_THETA_BASE, scale, beta)
    res = KH.refine_select(0, p, f, 12, h, 1, theta=theta, beta=beta)
    res.assert_guards()
    for b in safe[:3]:
        assert ((res["kind"][b] & 3) == 1).any(), (b, "a row with a NaN score was gated")
    assert not ((res["kind"][safe[3]] & 3) == 1).any()      # the untouched neighbour still gates
    check_select(res, p, f, [theta] * R.GATE_B, [beta] * R.GATE_B, [0.0] * R.GATE_B, h, 12, 1)


# ---- plan of the refine pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", R.RPLAN_K)
@pytest.mark.parametrize("pattern", R.RPLAN_PATTERNS)
def test_refine_plan(K, pattern):
    clen, trunk, lst, count = R.rplan_inputs(K, pattern)
    B = clen.shape[0]
    ref = R.refine_plan(clen, trunk, lst, count)
    res = KH.refine_plan(clen, trunk, lst, count)
    res.assert_guards()
    for name in ("count_off", "own_len", "own_off", "img_max", "totals"):
        eq(res[name], ref[name], name)
    for name in ("pre_len", "seg_src", "seg_pos0", "pre_off", "rlist", "eos_idx"):
        eq_or_untouched(res[name], ref[name], name)
    assert KH.untouched(res["eos_idx"][ref["R"]:]).all() and KH.untouched(res["rlist"][ref["R"]:]).all()
    assert (res["own_len"][B + B * ref["Kr"]:] == 0).all()      # the engine's memset, not the pattern


# ---- exact cosines ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", R.COMB_K)
@pytest.mark.parametrize("D", R.COMB_D)
def test_refine_cosine(K, D):
    feat, img, rlist, n = R.cosine_inputs(K, D)
    B = img.shape[0]
    res = KH.refine_cosine(feat, img, rlist, n, B, K)
    res.assert_guards()
    want = R.cosines(feat[:n], img, rlist[:n] // K)
    listed = np.zeros(B * K, bool)
    listed[rlist[:n]] = True
    assert KH.untouched(res["cos_out"])[~listed].all(), "a candidate outside rlist got a cosine"
    err = np.abs(res["cos_out"][rlist[:n]].astype(np.float64) - want).max()
    print(f"refine cosine K={K} D={D}: {n} rows, worst |d cos| {err:.2e}")
    assert err <= 2e-6
    assert (res["nonfinite"] == 0).all()


def test_refine_cosine_reports_a_nan_row_and_the_combine_keeps_the_guard_out_of_it():
    K, D = 200, 64
    feat, img, rlist, n = R.cosine_inputs(K, D)
    cos_in, rcos, probs, kind, guard = R.comb_inputs(K)
    # one image: its re-encoded candidates are those of combine row 0; a sampled candidate's features are NaN
    flat = np.nonzero(kind[0])[0].astype(np.int32)
    rng = np.random.default_rng(9)
    ft = rng.standard_normal((flat.size + 3, D)).astype(np.float32)
    bad = int(np.nonzero((kind[0][flat] & 3) == 2)[0][1])
    ft[bad] = np.nan
    rl = np.concatenate([flat, [-1, -1, -1]]).astype(np.int32)
    res = KH.refine_cosine(ft, img[:1], rl, flat.size, 1, K)
    res.assert_guards()
    assert res["nonfinite"][0] == 1 and (res["nonfinite"][1:] == 0).all()
    assert np.isnan(res["cos_out"][flat[bad]]) and np.isfinite(np.delete(res["cos_out"][flat], bad)).all()
    out = KH.combine_refine(cos_in[:1], probs[:1], R.COMB_LOGIT_SCALE, hyper(R.COMB_BETA), kind[:1], res["cos_out"][None, :], guard)
    out.assert_guards()
    assert (out["nonfinite"] == 0).all(), out["nonfinite"]      # no deviation recorded, no trip counted


# ---- the refine branch of the final combine ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", R.COMB_K)
def test_combine_refine(K):
    cos_in, rcos, probs, kind, guard = R.comb_inputs(K)
    B = R.COMB_B
    scale = float(np.exp(R.COMB_LOGIT_SCALE))
    ref = R.combine_refine(cos_in, probs, R.COMB_ALPHA, R.COMB_BETA, scale, kind, rcos, guard)
    res = KH.combine_refine(cos_in, probs, R.COMB_LOGIT_SCALE, hyper(R.COMB_BETA), kind, rcos, guard)
    res.assert_guards()
    cr, cs, fs = (res[n].reshape(B, K).astype(np.float64) for n in ("clip_ref", "clip_score", "final_score"))
    dev = float(res["nonfinite"][1:2].view(np.float32)[0])
    print(f"combine refine K={K}: worst |d clip_ref| {np.abs(cr - ref['clip_ref']).max():.2e}, |d clip_score| "
          f"{np.abs(cs - ref['clip_score']).max():.2e}, |d final_score| {np.abs(fs - ref['final']).max():.2e}, "
          f"|d best_cos| {np.abs(res['best_cos'] - ref['best_cos']).max():.2e}, |d dev| {abs(dev - ref['max_dev']):.2e} "
          f"(dev {ref['max_dev']:.3e}, guard {float(guard):.3e}, trips {ref['trips']})")
    np.testing.assert_allclose(cr, ref["clip_ref"], atol=2e-6, rtol=0)
    np.testing.assert_allclose(cs, ref["clip_score"], atol=2e-6, rtol=2e-4)
    np.testing.assert_allclose(fs, ref["final"], atol=1e-5, rtol=2e-4)
    np.testing.assert_allclose(res["best_cos"], ref["best_cos"], atol=2e-6, rtol=0)
    clear = ref["top2_gap"] > 1e-5
    eq(res["best"][clear], ref["best"][clear], "best")
    assert abs(dev - ref["max_dev"]) <= 5e-7
    assert res["nonfinite"][2] == ref["trips"]
    assert res["nonfinite"][0] == 0 and (res["nonfinite"][3:] == 0).all()
