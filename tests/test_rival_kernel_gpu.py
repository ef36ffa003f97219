"""-m gpu: the rival cosine kernel and the RIVAL instantiation of the combine kernel (conzic_amd/csrc/combine.hip) through the
hook czc_test_combine_rivals, against the NumPy float64 reference of tests/rival_ref.py.

Bars.  disc: |disc - ref| <= exp(logit_scale) * 1e-6 -- derived in rival_ref.py from the project's 2e-6 bar on an fp32 cosine,
not tuned.  final_score: that bar times |delta| plus the tolerance tests/test_kernels_gpu.py::test_fused_score_combine holds
the combine to (1e-5 + 2e-4 |ref|).  Worst |disc - ref| seen on the MI355X over all shapes (every test prints its own, -s):
1.2e-6 at exp(logit_scale) = 100 (bar 1e-4) and 2.8e-7 at 14.3 (bar 1.4e-5), 2 % of the bar at the worst."""
import numpy as np
import pytest

import draw_ref
import kernel_hooks as KH
import rival_hooks as RH
import rival_ref as RR
from conzic_amd import engine as E

pytestmark = pytest.mark.gpu

LOGIT_SCALES = (2.6592, float(np.log(100.0)))
N_IMG = 20
WORST = {"disc": 0.0}


def _inputs(K, M, D, seed=0):
    """B = 3 rows with m_b = 0, 1 and M rivals, own images 2, 0 and 5 of N_IMG."""
    rng = np.random.default_rng(7919 * K + 31 * M + D + seed)
    B = 3
    tf = rng.standard_normal((B * K, D)).astype(np.float32)
    ia = rng.standard_normal((N_IMG, D)).astype(np.float32)
    lg = rng.standard_normal((B, K)) * 2.0
    pr = np.exp(lg - lg.max(axis=1, keepdims=True))
    pr = (pr / pr.sum(axis=1, keepdims=True)).astype(np.float32)
    ior = np.array([2, 0, 5], np.int32)
    rv = np.full((B, M), -1, np.int32)
    rv[1, 0] = 9
    rv[2, :] = [i for i in rng.permutation(N_IMG) if i != 5][:M]
    return tf, ia, pr, ior, rv


def _hypers(B, alpha=0.02, beta=2.0):
    return [E.Engine.hyper(alpha, beta, 0.1) for _ in range(B)]


def _check_disc(got, ref, scale):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    bar = RR.disc_bar(scale)
    WORST["disc"] = max(WORST["disc"], err / bar)
    print(f"worst |disc - ref| = {err:.3e} (bar {bar:.3e}); worst so far {WORST['disc']:.3f} of the bar")
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("D", [64, 96, 512])
@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("K", [1, 5, 200, 1024])
def test_rival_combine_against_fp64(K, M, D):
    tf, ia, pr, ior, rv = _inputs(K, M, D)
    delta = np.array([0.5, 0.5, 1.5], np.float32)
    B = 3
    for ls in LOGIT_SCALES:
        g = RH.combine_rivals(tf, ia, ior, rv, delta, ls, pr, _hypers(B))
        g.assert_guards()
        assert not KH.untouched(g["clip_ref"]).any() and not KH.untouched(g["disc"]).any() and not KH.untouched(g["final_score"]).any()
        assert g["nonfinite"][0] == 0
        ref = RR.combine(tf, ia, ior, rv, delta, ls, pr, 0.02, 2.0)
        # the cosines: the bits of the kernel every other call uses
        _, cr, _, _ = KH.combine(tf, ia[ior], ls, pr, E.Engine.hyper(0.02, 2.0, 0.1))
        assert np.array_equal(g["clip_ref"].view(np.uint32), cr.view(np.uint32))
        np.testing.assert_allclose(g["clip_ref"], ref["cos"], atol=2e-6)
        _check_disc(g["disc"], ref["disc"], ref["scale"])
        assert np.all(g["disc"][0] == 1.0)   # no rival: exactly 1
        tol = 1e-5 + 2e-4 * np.abs(ref["final0"]) + np.abs(delta.astype(np.float64))[:, None] * RR.disc_bar(ref["scale"])
        assert np.all(np.abs(g["final_score"].astype(np.float64) - ref["final"]) <= tol)
        sure = RR.top2_margin(ref["final"]) > 2 * tol.max(axis=1)
        assert np.array_equal(g["best"][sure], ref["final"].argmax(axis=1)[sure])
        assert sure.any() or K == 1


def test_planted_rivals():
    K, M, D = 200, 3, 512
    tf, ia, pr, ior, rv = _inputs(K, M, D, seed=1)
    ls = LOGIT_SCALES[1]
    B = 3
    delta = np.ones(B, np.float32)
    # row 1: its one rival is a copy of its own image (another index, the same embedding): disc = 1/2 for every k
    ia[9] = ia[ior[1]]
    # row 2: candidates close to the own image, rivals unrelated: every cj far below c0, disc -> 1
    tf[2 * K:3 * K] = ia[ior[2]][None, :] + 0.05 * tf[2 * K:3 * K]
    g = RH.combine_rivals(tf, ia, ior, rv, delta, ls, pr, _hypers(B))
    g.assert_guards()
    ref = RR.combine(tf, ia, ior, rv, delta, ls, pr, 0.02, 2.0)
    _check_disc(g["disc"], ref["disc"], ref["scale"])
    assert np.all(np.abs(g["disc"][1].astype(np.float64) - 0.5) <= RR.disc_bar(ref["scale"]))
    assert np.all(g["disc"][2] > 1.0 - 1e-6) and np.all(g["disc"][2] <= 1.0)


def test_scaled_features_keep_the_cosine_bits():
    """Features a thousand times larger: the rival kernel's c0 still has the bits of the cosine kernel on the same features, and
    nothing overflows."""
    K, M, D = 5, 3, 96
    tf, ia, pr, ior, rv = _inputs(K, M, D, seed=2)
    tf = (tf * np.float32(1e3)).astype(np.float32)
    for ls in LOGIT_SCALES:
        g = RH.combine_rivals(tf, ia, ior, rv, np.ones(3, np.float32), ls, pr, _hypers(3))
        _, cr, _, _ = KH.combine(tf, ia[ior], ls, pr, E.Engine.hyper(0.02, 2.0, 0.1))
        assert np.array_equal(g["clip_ref"].view(np.uint32), cr.view(np.uint32))
        assert g["nonfinite"][0] == 0 and np.isfinite(g["disc"]).all()
        ref = RR.combine(tf, ia, ior, rv, np.ones(3), ls, pr, 0.02, 2.0)
        _check_disc(g["disc"], ref["disc"], ref["scale"])


@pytest.mark.parametrize("where", ["feature", "rival"])
def test_nonfinite_raises_the_flag(where):
    K, M, D = 5, 3, 64
    tf, ia, pr, ior, rv = _inputs(K, M, D, seed=3)
    if where == "feature":
        tf[2 * K + 1, 7] = np.nan
    else:
        ia[rv[2, 1], 3] = np.nan   # a rival image of row 2 only: c0 stays finite everywhere
    g = RH.combine_rivals(tf, ia, ior, rv, np.ones(3, np.float32), LOGIT_SCALES[0], pr, _hypers(3))
    g.assert_guards()
    assert g["nonfinite"][0] == 1
    if where == "rival":
        assert np.isfinite(g["clip_ref"]).all()


def test_rows_wider_than_the_lds_array_are_refused():
    """D * CZC_MAX_RIVALS * 4 beyond the kernel's 32 KB LDS array (D > 512), and M outside [1, 16]: refused before any launch."""
    from conzic_amd import native
    tf, ia, pr, ior, rv = _inputs(5, 3, 576)
    with pytest.raises(native.NativeError) as ei:
        RH.combine_rivals(tf, ia, ior, rv, np.ones(3, np.float32), LOGIT_SCALES[0], pr, _hypers(3))
    assert ei.value.code == native.ERR_ARG
    tf, ia, pr, ior, rv = _inputs(5, 3, 64)
    with pytest.raises(native.NativeError) as ei:
        RH.combine_rivals(tf, ia, ior, np.full((3, 17), -1, np.int32), np.ones(3, np.float32), LOGIT_SCALES[0], pr, _hypers(3))
    assert ei.value.code == native.ERR_ARG


@pytest.mark.parametrize("K,D", [(5, 64), (200, 512)])
def test_skipped_term_keeps_the_bits(K, D):
    """A row with delta = 0, or without a rival, inside a launch that has an active row: final_score has the bits of the
    czc_test_combine_draw hook (no rivals anywhere).  The active row moves, so the term is not ignored."""
    M = 3
    tf, ia, pr, ior, rv = _inputs(K, M, D, seed=4)
    rv[1, :] = [3, 4, 6]                          # row 1 has rivals but delta 0; row 0 has delta but no rival; row 2 has both
    delta = np.array([0.7, 0.0, 0.7], np.float32)
    seeds = np.array([11, 12, 13], np.uint64)
    for ls in LOGIT_SCALES:
        for taus in (0.0, 0.5):
            draws = draw_ref.make_draws(seeds, taus)
            g = RH.combine_rivals(tf, ia, ior, rv, delta, ls, pr, _hypers(3), draws=draws, step=3)
            g.assert_guards()
            fs, best = draw_ref.combine_draw(tf, ia[ior], ls, pr, E.Engine.hyper(0.02, 2.0, 0.1), draws, 3)
            for b in (0, 1):
                assert np.array_equal(g["final_score"][b].view(np.uint32), fs[b].view(np.uint32)), (ls, taus, b)
                assert g["best"][b] == best[b]
            assert not np.array_equal(g["final_score"][2], fs[2])
            np.testing.assert_allclose(g["final_score"][2].astype(np.float64) - fs[2], 0.7 * g["disc"][2].astype(np.float64), atol=1e-6)
