"""-m gpu: the score-combine kernel (conzic_amd/csrc/combine.hip) in every instantiation without rivals, through the hook
czc_test_combine_rows (tests/combine_hooks.py), against the NumPy float64 reference and the DERIVED bars of tests/combine_ref.py
(its module docstring has the derivation; nothing here is tuned to what the kernel returns).  Every comparison prints worst / bar.

Worst error / bar seen on the MI355X over all cases of this file (pytest -s prints each case's own):
    cosine-input mode    clip_score 0.45 (K 511, s 100)   clip_ref 0.50 (one rounding of the two allowed)   final_score 0.94 (K 1000, s 100)
    feature-input mode   clip_score 0.03                  clip_ref 0.04 of 2e-6                             final_score 0.89 (B 257, K 8)
    mixed rows (form 2)  clip_score 0.45                  clip_ref 0.50                                     final_score 0.76
    czc_similarity       clip_score 0.02                  clip_ref 0.03
final_score comes close to its bar where the softmax term is negligible and the score is alpha * probs alone: two roundings allowed,
two taken.  No row of any of the 148 compared cases fell below the winner margin; no draw was a near tie.
Against exp(logit_scale) in float64 instead of the fp32 scale the kernel is handed (combine_ref.py (b)) clip_score reaches 1.01 of
this bar at s = 100: the scale's own rounding, not the kernel's arithmetic."""
import numpy as np
import pytest

import combine_hooks as CH
import combine_ref as CR
import draw_ref
import kernel_hooks as KH
from conzic_amd import native

pytestmark = pytest.mark.gpu

WORST = {}
OUTS = ("clip_score", "clip_ref", "final_score", "best", "best_cos")


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


def _whole(g, names=CH.FLOATS + ("best", "best_cos")):
    g.assert_guards()
    for n in names:
        assert not KH.untouched(g[n]).any(), n


def _same_bits(a, b, names=OUTS, rows=None, rows_b=None):
    for n in names:
        x = CH.bits(a[n]) if rows is None else CH.bits(a[n])[rows]
        y = CH.bits(b[n]) if rows_b is None else CH.bits(b[n])[rows_b]
        assert np.array_equal(x, y), n


def _against_fp64(tag, g, r, b, K):
    """clip_score, clip_ref, final_score inside their bars; best on the rows the reference is sure of; best_cos the winner's clip_ref"""
    for name, got, ref, bar in (("clip_score", g["clip_score"], r.clip_score, b.clip_score), ("clip_ref", g["clip_ref"], r.clip_ref, b.clip_ref),
                                ("final_score", g["final_score"], r.final, b.final)):
        ratio = float((np.abs(got.astype(np.float64) - ref) / bar).max())
        _note(name, ratio)
        print(f"[combine] {tag} {name}: worst / bar = {ratio:.3f} (all cases so far {WORST[name]:.3f})")
        assert ratio <= 1.0, (tag, name, ratio)
    sure = CR.sure_rows(r, b)
    print(f"[combine] {tag}: {1.0 - sure.mean():.3f} of the rows left out of the winner comparison")
    assert 1.0 - sure.mean() <= CR.MAX_LEFT_OUT and (sure.any() or K == 1)
    assert ((g["best"] >= 0) & (g["best"] < K)).all()
    assert np.array_equal(g["best"][sure], r.best[sure]), tag
    rows = np.arange(g["best"].size)
    assert np.array_equal(CH.bits(g["best_cos"]), CH.bits(g["clip_ref"][rows, g["best"]]))
    assert not g["nonfinite"].any()


def _hyper_of(control):
    return CH.hyper(*CR.CONTROL_HYPER[control], control)


# ---- 1. cosine-input mode against fp64 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("control", [0, 1, 2])
@pytest.mark.parametrize("K", CR.COS_KS)
def test_cosine_input_against_fp64(K, control):
    for ls in CR.LOGIT_SCALES:
        for span in ((False, True) if K >= 2 else (False,)):
            case = CR.cos_case(K, control, span=span)
            refused, g = CH.combine_rows(ls, case["probs"], _hyper_of(control), cos=case["cos"], cand=case["cand"],
                                         senti_raw=case["senti_raw"], repeats=case["repeats"])
            assert not refused
            _whole(g)
            r, b = CR.case_ref(case, ls, control, scale=g.scale)
            _against_fp64(f"cos K {K} control {control} s {r.scale:.1f} span {int(span)}", g, r, b, K)


# ---- 2. feature-input mode ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,D,B", [(K, D, CR.FEAT_B) for K in CR.FEAT_KS for D in CR.FEAT_DS] + [(CR.FEAT_WIDE[1], CR.FEAT_WIDE[2], CR.FEAT_WIDE[0])])
def test_feature_input_against_fp64(K, D, B):
    case = CR.feat_case(K, D, B=B)
    for ls in CR.LOGIT_SCALES:
        refused, g = CH.combine_rows(ls, case["probs"], _hyper_of(0), text_feat=case["text_feat"], img=case["img"], cand=case["cand"])
        assert not refused
        _whole(g)
        r, b = CR.case_ref(case, ls, 0, feature_mode=True, scale=g.scale)
        _against_fp64(f"feat K {K} D {D} B {B} s {r.scale:.1f}", g, r, b, K)
        _, cr, _, _ = KH.combine(case["text_feat"], case["img"], ls, case["probs"], _hyper_of(0))   # the same cosine kernel
        assert np.array_equal(CH.bits(g["clip_ref"]), CH.bits(cr))


# ---- 3. every form gives the scalar form's bits -------------------------------------------------------------------------------------

@pytest.mark.parametrize("control", [0, 1, 2])
@pytest.mark.parametrize("K", [5, 257])
def test_every_form_gives_the_scalar_forms_bits(K, control):
    case = CR.cos_case(K, control, seed=3)
    B = case["probs"].shape[0]
    h = _hyper_of(control)
    kw = dict(cos=case["cos"], cand=case["cand"], senti_raw=case["senti_raw"], repeats=case["repeats"])
    for ls in CR.LOGIT_SCALES:
        _, g0 = CH.combine_rows(ls, case["probs"], h, form=0, **kw)
        _whole(g0)
        for form in (1, 2, 3):
            hs = h if form == 1 else [h] * B
            draws = draw_ref.make_draws(np.arange(B) + 5, 0.0) if form == 3 else None
            refused, g = CH.combine_rows(ls, case["probs"], hs, form=form, draws=draws, step=4, **kw)
            assert not refused
            _whole(g)
            _same_bits(g, g0)


# ---- 4. mixed rows in one launch ----------------------------------------------------------------------------------------------------

def _mixed(B, K, seed=4):
    """CR.mixed_case with its hyper-parameters as records"""
    tuples, case = CR.mixed_case(B, K, seed=seed)
    return tuples, [CH.hyper(*t) for t in tuples], case


@pytest.mark.parametrize("K", CR.MIXED_KS)
def test_mixed_rows_in_one_launch(K):
    B = CR.MIXED_B
    tuples, hs, case = _mixed(B, K)
    assert {h.alpha for h in hs} == {float(np.float32(a)) for a in CR.ALPHAS} and {h.control for h in hs} == {0, 1, 2}
    assert len({h.beta for h in hs}) == 3 and len({h.gamma for h in hs}) == 3
    kw = lambda rows: dict(cos=case["cos"][rows], cand=case["cand"][rows], senti_raw=case["senti_raw"][rows], repeats=case["repeats"][rows])
    for ls in CR.LOGIT_SCALES:
        refused, g = CH.combine_rows(ls, case["probs"], hs, form=2, **kw(slice(None)))
        assert not refused
        _whole(g)
        r, b = CR.mixed_ref(tuples, case, ls, scale=g.scale)
        _against_fp64(f"mixed K {K} s {r.scale:.1f}", g, r, b, K)
        for i in range(B):   # the row alone, in the scalar form, with its own scalars
            _, g1 = CH.combine_rows(ls, case["probs"][i:i + 1], hs[i], form=0, **kw(slice(i, i + 1)))
            _same_bits(g, g1, rows=slice(i, i + 1))
        perm = np.random.default_rng(K).permutation(B)
        _, gp = CH.combine_rows(ls, case["probs"][perm], [hs[i] for i in perm], form=2, **kw(perm))
        _same_bits(gp, g, rows_b=perm)


# ---- 5. unused control inputs are never read ----------------------------------------------------------------------------------------

def test_unused_control_inputs_are_never_read():
    K = 257
    case = CR.cos_case(K, 1, seed=5)
    B = case["probs"].shape[0]
    nan = np.full((B, K), np.nan, np.float32)
    ls = CR.LOGIT_SCALES[1]
    # scalar form, control 0: NaN arrays against null arrays
    _, g0 = CH.combine_rows(ls, case["probs"], _hyper_of(0), cos=case["cos"])
    _, gn = CH.combine_rows(ls, case["probs"], _hyper_of(0), cos=case["cos"], senti_raw=nan, repeats=nan)
    _same_bits(gn, g0)
    assert np.isfinite(gn["final_score"]).all() and not gn["nonfinite"].any()
    # scalar form, control 2: NaN repeats against null repeats
    pos = CR.cos_case(K, 2, seed=5)
    _, g2 = CH.combine_rows(ls, pos["probs"], _hyper_of(2), cos=pos["cos"], senti_raw=pos["senti_raw"])
    _, g2n = CH.combine_rows(ls, pos["probs"], _hyper_of(2), cos=pos["cos"], senti_raw=pos["senti_raw"], repeats=nan)
    _same_bits(g2n, g2)
    assert np.isfinite(g2n["final_score"]).all() and not g2n["nonfinite"].any()
    # per row: control-0 rows with NaN in both arrays, control-2 rows with NaN in repeats
    _, hs, mixed = _mixed(9, K, seed=6)
    ctl = np.arange(9) % 3
    sr, rp = mixed["senti_raw"].copy(), mixed["repeats"].copy()
    sr[ctl == 0] = np.nan
    rp[ctl != 1] = np.nan
    _, gc = CH.combine_rows(ls, mixed["probs"], hs, form=2, cos=mixed["cos"], senti_raw=mixed["senti_raw"], repeats=mixed["repeats"])
    _, gd = CH.combine_rows(ls, mixed["probs"], hs, form=2, cos=mixed["cos"], senti_raw=sr, repeats=rp)
    _same_bits(gd, gc)
    assert np.isfinite(gd["final_score"]).all() and not gd["nonfinite"].any()


# ---- 6. mixed hypers with the draw --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [8, 257])
def test_mixed_hypers_with_the_draw(K):
    B = 36
    _, hs, case = _mixed(B, K, seed=7)
    seeds = np.random.default_rng(K).integers(0, 2 ** 64, size=B, dtype=np.uint64)
    taus = np.where(np.arange(B) % 4 == 0, 0.0, np.where(np.arange(B) % 2 == 0, 0.05, 0.5)).astype(np.float32)
    kw = dict(cos=case["cos"], cand=case["cand"], senti_raw=case["senti_raw"], repeats=case["repeats"])
    ls = CR.LOGIT_SCALES[0]
    _, g2 = CH.combine_rows(ls, case["probs"], hs, form=2, **kw)
    moved = 0
    for step0, step in ((0, 0), (3, 4)):
        refused, g3 = CH.combine_rows(ls, case["probs"], hs, form=3, draws=draw_ref.make_draws(seeds, taus, step0=step0), step=step, **kw)
        assert not refused
        _whole(g3)
        _same_bits(g3, g2, names=CH.FLOATS)
        want, tie = draw_ref.winners(g3["final_score"], case["probs"], seeds, taus, step0 + step)
        print(f"[combine] draw K {K} step {step0 + step}: {int(tie.sum())} near ties of {B}")
        assert tie.mean() <= draw_ref.NEAR_TIE_CAP
        assert np.array_equal(g3["best"][~tie], want[~tie])
        assert np.array_equal(g3["best"][taus == 0], g2["best"][taus == 0])
        rows = np.arange(B)
        assert np.array_equal(CH.bits(g3["best_cos"]), CH.bits(g3["clip_ref"][rows, g3["best"]]))
        moved += int((g3["best"] != g2["best"]).sum())
    assert moved > 0   # the draw is not the argmax


# ---- 7. write-back ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 7, 77])
def test_write_back(T):
    B, K = 5, 63
    case = CR.cos_case(K, 0, B=B, seed=8)
    inp = (100000 + 1000 * np.arange(B)[:, None] + np.arange(T)[None, :]).astype(np.int32)
    assert case["cand"].min() >= 1 and case["cand"].max() < 30522
    ls = CR.LOGIT_SCALES[0]
    h = _hyper_of(0)
    _, g0 = CH.combine_rows(ls, case["probs"], h, cos=case["cos"], cand=case["cand"])   # inp NULL: nothing to write
    assert "inp" not in g0

    def check(g, cols):
        _whole(g, CH.FLOATS + ("best", "best_cos", "inp"))
        _same_bits(g, g0)
        want = CR.write_back(inp, case["cand"], g["best"], cols)
        assert np.array_equal(g["inp"], want)
        assert ((g["inp"] != inp).sum(axis=1) == 1).all()   # one word per row: ids are below the pattern's values

    for col in sorted({0, T - 1}):
        _, g = CH.combine_rows(ls, case["probs"], h, cos=case["cos"], cand=case["cand"], inp=inp, gen_idx=col)
        check(g, col)
    cols = np.array([0, T - 1, T // 2, T - 1, 0], np.int32)
    for form in (1, 2, 3):
        hs = h if form == 1 else [h] * B
        draws = draw_ref.make_draws(np.arange(B), 0.0) if form == 3 else None
        _, g = CH.combine_rows(ls, case["probs"], hs, form=form, draws=draws, cos=case["cos"], cand=case["cand"], inp=inp, gen_rows=cols,
                               gen_idx=T // 3)
        check(g, cols)


# ---- 8. ties and the first argmax ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,at", [(1024, (700, 44, 300)), (257, (255, 256)), (64, tuple(range(64)))])
def test_ties_take_the_first_index(K, at):
    case = CR.planted_ties(K, at)
    for ls in CR.LOGIT_SCALES:
        for form in (0, 2):
            hs = _hyper_of(0) if form == 0 else [_hyper_of(0)] * 3
            _, g = CH.combine_rows(ls, case["probs"], hs, form=form, cos=case["cos"], cand=case["cand"])
            _whole(g)
            f = g["final_score"]
            assert (CH.bits(f[:, list(at)]) == CH.bits(f.max(axis=1, keepdims=True))).all()   # equal inputs, equal scores: an exact tie
            assert ((f == f.max(axis=1, keepdims=True)).sum(axis=1) == len(at)).all()
            assert (g["best"] == min(at)).all()


def test_dominant_winner():
    case = CR.dominant_winner(200, 137)
    _, g = CH.combine_rows(CR.LOGIT_SCALES[1], case["probs"], _hyper_of(0), cos=case["cos"], cand=case["cand"])
    assert (g["best"] == 137).all()


# ---- 9. non-finite inputs -----------------------------------------------------------------------------------------------------------

def test_nonfinite_inputs_raise_the_flag():
    K, D, B = 5, 64, 4
    case = CR.feat_case(K, D, B=B, seed=9)
    ls = CR.LOGIT_SCALES[0]
    call = lambda tf: CH.combine_rows(ls, case["probs"], _hyper_of(0), text_feat=tf, img=case["img"], cand=case["cand"])[1]
    g0 = call(case["text_feat"])
    assert not g0["nonfinite"].any()
    others = np.array([0, 2, 3])
    for what in ("one NaN element", "a zero row", "an all-NaN image row"):
        tf = case["text_feat"].copy()
        if what == "one NaN element":
            tf[1 * K + 2, 7] = np.nan
        elif what == "a zero row":
            tf[1 * K + 2] = 0.0     # 0 / 0
        else:
            tf[1 * K:2 * K] = np.nan
        g = call(tf)
        _whole(g)
        assert g["nonfinite"][0] == 1 and not g["nonfinite"][1:].any(), what
        assert ((g["best"] >= 0) & (g["best"] < K)).all()
        _same_bits(g, g0, rows=others, rows_b=others)
        assert np.isnan(g["clip_ref"][1, 2])
        if what == "an all-NaN image row":
            assert g["best"][1] == 0


# ---- 10. refusal --------------------------------------------------------------------------------------------------------------------

def test_refusal_and_argument_checks():
    ls = CR.LOGIT_SCALES[0]
    K, B = 1025, 2
    rng = np.random.default_rng(10)
    pr = CR.fluency(rng, B, K)
    cos = rng.uniform(-0.4, 0.4, (B, K)).astype(np.float32)
    inp = np.arange(B * 3, dtype=np.int32).reshape(B, 3) + 7
    refused, g = CH.combine_rows(ls, pr, _hyper_of(0), text_feat=rng.standard_normal((B * K, 8)), img=rng.standard_normal((B, 8)), inp=inp)
    assert refused
    g.assert_guards()
    for n in OUTS:
        assert KH.untouched(g[n]).all(), n
    assert np.array_equal(g["inp"], inp) and not g["nonfinite"].any()
    refused, g = CH.combine_rows(ls, pr, [_hyper_of(0)] * B, form=2, cos=cos)
    assert refused
    for n in ("clip_score", "final_score", "best", "best_cos"):
        assert KH.untouched(g[n]).all(), n
    assert np.array_equal(CH.bits(g["clip_ref"]), CH.bits(cos))   # the cosines as they were placed there

    case = CR.cos_case(5, 1, seed=10)
    B = case["probs"].shape[0]
    T = 4
    inp = np.zeros((B, T), np.int32)
    ok = dict(cos=case["cos"], cand=case["cand"], inp=inp)
    hs = [_hyper_of(1)] * B
    bad_calls = [
        dict(ok, hypers=_hyper_of(0), gen_idx=T),
        dict(ok, hypers=_hyper_of(0), gen_idx=-1),
        dict(ok, hypers=_hyper_of(0), form=1, gen_rows=[0, 1, T, 2]),
        dict(ok, hypers=_hyper_of(0), form=1, gen_rows=[0, -1, 1, 2]),
        dict(ok, hypers=_hyper_of(1), senti_raw=case["senti_raw"]),                          # control 1 without repeats
        dict(ok, hypers=[_hyper_of(0)] * 3 + [_hyper_of(1)], form=2, gen_rows=[0] * B, senti_raw=case["senti_raw"]),
        dict(ok, hypers=_hyper_of(2)),                                                        # control 2 without scores
        dict(ok, hypers=hs, form=2, gen_rows=[0] * B, senti_raw=case["senti_raw"], repeats=case["repeats"], run=[0, 1, 2, B]),
        dict(ok, hypers=hs, form=2, gen_rows=[0] * B, senti_raw=case["senti_raw"], repeats=case["repeats"], run=[0, -1, 2, 3]),
    ]
    for kw in bad_calls:
        kw = dict(kw)
        h = kw.pop("hypers")
        with pytest.raises(native.NativeError) as ei:
            CH.combine_rows(ls, case["probs"], h, **kw)
        assert ei.value.code == native.ERR_ARG
        refused, g = CH.combine_rows(ls, case["probs"], _hyper_of(1), senti_raw=case["senti_raw"], repeats=case["repeats"], gen_idx=T - 1, **ok)
        assert not refused
        _whole(g)
        assert np.array_equal(g["inp"], CR.write_back(inp, case["cand"], g["best"], T - 1))


# ---- 11. compact batches ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", [[5, 0, 3], [6], list(range(8)), [7, 7, 1, 0, 2]])
def test_compact_batches_read_the_gathered_records(run):
    R, K, T = 8, 65, 6
    _, hs, case = _mixed(R, K, seed=11)
    seeds = np.arange(R, dtype=np.uint64) * 977 + 3
    draws = draw_ref.make_draws(seeds, np.where(np.arange(R) % 2 == 0, 0.5, 0.0), step0=2)
    cols = (np.arange(R) % T).astype(np.int32)
    inp = (100000 + 100 * np.arange(R)[:, None] + np.arange(T)[None, :]).astype(np.int32)
    ls = CR.LOGIT_SCALES[1]
    run = np.asarray(run)
    data = lambda rows: dict(cos=case["cos"][rows], cand=case["cand"][rows], senti_raw=case["senti_raw"][rows], repeats=case["repeats"][rows],
                             gen_rows=cols[rows], inp=inp[rows])
    from conzic_amd.engine import draw_array, hyper_array
    for form in (2, 3):
        dr = draws if form == 3 else None
        _, full = CH.combine_rows(ls, case["probs"], hs, form=form, draws=dr, step=1, **data(slice(None)))
        refused, g = CH.combine_rows(ls, case["probs"][run], hs, form=form, draws=dr, step=1, run=run, **data(run))
        assert not refused
        _whole(g, CH.FLOATS + ("best", "best_cos", "inp", "hp") + (("draw",) if form == 3 else ()))
        _same_bits(g, full, names=OUTS + ("inp",), rows_b=run)
        assert np.array_equal(g["hp"], CH.record_words(hyper_array(hs))[run])
        if form == 3:
            assert np.array_equal(g["draw"], CH.record_words(draw_array(draws))[run])


# ---- 12. czc_similarity -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny_engine():
    from conzic_amd import harness
    su = harness.build_synthetic(True, native.PREC_F32)
    assert su.clip_cfg.proj == 64
    yield su.engine, float(su.clip_cfg.logit_scale)
    su.engine.close()


@pytest.mark.parametrize("K", [1, 200])
def test_similarity_is_the_combine_with_beta_one(tiny_engine, K):
    eng, ls = tiny_engine
    case = CR.feat_case(K, 64, B=3, seed=12)
    cs, cr = eng.similarity(case["img"], case["text_feat"], K)
    _, g = CH.combine_rows(ls, np.zeros((3, K), np.float32), CH.hyper(0.0, 1.0), text_feat=case["text_feat"], img=case["img"])
    assert np.array_equal(CH.bits(cs), CH.bits(g["clip_score"])) and np.array_equal(CH.bits(cr), CH.bits(g["clip_ref"]))
    r = CR.combine((case["text_feat"], case["img"]), ls, np.zeros((3, K)), 0.0, 1.0, scale=g.scale)   # the engine's scale: same bits
    b = CR.bars(r, feature_mode=True)
    for name, got, ref, bar in (("clip_score", cs, r.clip_score, b.clip_score), ("clip_ref", cr, r.clip_ref, b.clip_ref)):
        ratio = float((np.abs(got.astype(np.float64) - ref) / bar).max())
        _note(name, ratio)
        print(f"[combine] similarity K {K} {name}: worst / bar = {ratio:.3f}")
        assert ratio <= 1.0


def test_similarity_refuses_k_out_of_range(tiny_engine):
    eng, _ = tiny_engine
    K = native.MAX_TOPK + 1
    case = CR.feat_case(2, 64, B=1, seed=13)
    big = np.zeros((K, 64), np.float32)
    out = np.empty((1, K), np.float32)
    for k in (K, 0):
        rc = eng.lib.czc_similarity(eng.h, case["img"].ctypes.data, big.ctypes.data, 1, k, out.ctypes.data, out.ctypes.data)
        assert rc == native.ERR_ARG
    cs, cr = eng.similarity(case["img"], case["text_feat"], 2)   # the engine is still usable
    assert np.isfinite(cs).all() and abs(float(cs.sum()) - 1.0) < 1e-5 and np.isfinite(cr).all()
