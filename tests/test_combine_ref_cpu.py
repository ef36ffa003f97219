"""CPU self-tests of tests/combine_ref.py: the float64 reference against the torch formulas of oracle/, the input generators of
tests/test_combine_kernel_gpu.py against the winner rule (on the reference alone), the planted cases, and the bar functions."""
import numpy as np
import pytest
import torch

import combine_ref as CR
from oracle import models as M


def _torch_step(cos_or_feats, logit_scale, probs, alpha, beta, gamma, control, sraw, repeats):
    """oracle/models.py::clip_similarity and oracle/step.py::polish_step lines 210-226 in float64"""
    pr = torch.from_numpy(np.asarray(probs, np.float64))
    if isinstance(cos_or_feats, tuple):
        tf, ie = (torch.from_numpy(np.asarray(x, np.float64)) for x in cos_or_feats)
        clip_score, clip_ref = M.clip_similarity({"logit_scale": torch.tensor(logit_scale, dtype=torch.float64)}, ie, tf)
    else:
        scale = torch.tensor(logit_scale, dtype=torch.float64).exp()
        logits = torch.from_numpy(np.asarray(cos_or_feats, np.float64)) * scale
        clip_score, clip_ref = logits.softmax(dim=1), logits / scale
    final = alpha * pr + beta * clip_score
    if control == 2:
        final = final + gamma * torch.softmax(torch.from_numpy(np.asarray(sraw, np.float64)) / 0.1, dim=-1)
    elif control == 1:
        sprob = torch.softmax(torch.from_numpy(np.asarray(sraw, np.float64)) / 1, dim=1)
        final = final + gamma * sprob + 0.1 * (1 - torch.exp(torch.from_numpy(np.asarray(repeats, np.float64))))
    return clip_score.numpy(), clip_ref.numpy(), final.numpy(), final.argmax(dim=1).numpy()


@pytest.mark.parametrize("control", [0, 1, 2])
@pytest.mark.parametrize("feature_mode", [False, True])
def test_reference_is_the_oracle_formulas(control, feature_mode):
    for ls in CR.LOGIT_SCALES:
        case = CR.feat_case(7, 16, B=3, control=control) if feature_mode else CR.cos_case(9, control, B=3)
        al, be, ga = CR.CONTROL_HYPER[control]
        cos = (case["text_feat"], case["img"]) if feature_mode else case["cos"]
        r = CR.combine(cos, ls, case["probs"], al, be, ga, control, case["senti_raw"], case["repeats"])
        cs, cr, fin, best = _torch_step(cos, ls, case["probs"], al, be, ga, control, case["senti_raw"], case["repeats"])
        np.testing.assert_allclose(r.clip_score, cs, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(r.clip_ref, cr, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(r.final, fin, rtol=1e-12, atol=1e-15)
        np.testing.assert_array_equal(r.best, best)


def test_per_row_hypers_are_the_scalar_rows():
    """[B] alpha / beta / gamma / control give, row by row, what the scalar call gives on that row"""
    K = 11
    c1, c2 = CR.cos_case(K, 1, B=3), CR.cos_case(K, 2, B=3)
    sr = np.stack([c1["senti_raw"][0], c2["senti_raw"][1], c1["senti_raw"][2]])
    al, be, ga, ctl = [0.0, 0.02, 1.0], [2.0, 0.0, 1.0], [5.0, 0.5, 7.0], [1, 2, 0]
    r = CR.combine(c1["cos"], 2.6592, c1["probs"], al, be, ga, ctl, sr, c1["repeats"])
    for b in range(3):
        one = CR.combine(c1["cos"][b:b + 1], 2.6592, c1["probs"][b:b + 1], al[b], be[b], ga[b], ctl[b], sr[b:b + 1], c1["repeats"][b:b + 1])
        np.testing.assert_array_equal(r.final[b], one.final[0])
    assert not np.array_equal(r.final[2], CR.combine(c1["cos"], 2.6592, c1["probs"], 1.0, 1.0, 7.0, 1, sr, c1["repeats"]).final[2])


def _assert_share(tag, r, b, K):
    share, kept = CR.left_out(r, b)
    print(f"[combine_ref] {tag}: {share:.3f} of the rows left out, {kept} kept")
    assert share <= CR.MAX_LEFT_OUT, (tag, share)
    assert kept >= 1 or K == 1, tag


@pytest.mark.parametrize("control", [0, 1, 2])
@pytest.mark.parametrize("K", CR.COS_KS)
def test_cosine_cases_meet_the_winner_rule(K, control):
    for ls in CR.LOGIT_SCALES:
        for span in ((False, True) if K >= 2 else (False,)):
            case = CR.cos_case(K, control, span=span)
            r, b = CR.case_ref(case, ls, control)
            _assert_share(f"K {K} control {control} scale {ls:.4f} span {span}", r, b, K)
            if span:
                assert case["cos"].min() == -1.0 and case["cos"].max() == 1.0
            else:
                assert np.abs(case["cos"]).max() <= 0.4


@pytest.mark.parametrize("K,D,B", [(K, D, CR.FEAT_B) for K in CR.FEAT_KS for D in CR.FEAT_DS] + [(CR.FEAT_WIDE[1], CR.FEAT_WIDE[2], CR.FEAT_WIDE[0])])
def test_feature_cases_meet_the_winner_rule(K, D, B):
    for ls in CR.LOGIT_SCALES:
        r, b = CR.case_ref(CR.feat_case(K, D, B=B), ls, 0, feature_mode=True)
        _assert_share(f"K {K} D {D} B {B} scale {ls:.4f}", r, b, K)


@pytest.mark.parametrize("B,K,seed", [(CR.MIXED_B, K, 4) for K in CR.MIXED_KS])
def test_mixed_cases_meet_the_winner_rule(B, K, seed):
    """the one launch with mixed control signals: every alpha, beta, gamma and control occurs, neighbours differ in control, and the
    reference alone keeps the rows the winner comparison needs"""
    hs, case = CR.mixed_case(B, K, seed=seed)
    assert {h[0] for h in hs} == set(CR.ALPHAS) and {h[1] for h in hs} == set(CR.BETAS) and {h[2] for h in hs} == set(CR.GAMMAS)
    assert all(a[3] != b[3] for a, b in zip(hs, hs[1:])) and {h[3] for h in hs} == {0, 1, 2}
    assert all(h[0] or h[1] or h[2] for h in hs)
    for ls in CR.LOGIT_SCALES:
        r, b = CR.mixed_ref(hs, case, ls)
        _assert_share(f"mixed B {B} K {K} scale {ls:.4f}", r, b, K)


@pytest.mark.parametrize("K,at", [(1024, (700, 44, 300)), (257, (255, 256)), (64, tuple(range(64)))])
def test_planted_ties_tie_exactly(K, at):
    case = CR.planted_ties(K, at)
    for ls in CR.LOGIT_SCALES:
        r, _ = CR.case_ref(case, ls, 0)
        top = r.final.max(axis=1, keepdims=True)
        assert np.array_equal(np.nonzero(r.final[0] == top[0])[0], np.sort(at))
        assert (r.final[:, list(at)] == top).all() and r.top2_margin.max() == 0.0
        assert (r.best == min(at)).all()
        # equal fp32 inputs: the cosines and the fluencies of the tied columns are the same numbers
        assert np.unique(case["cos"][:, list(at)]).size == 1 and np.unique(case["probs"]).size == 1


def test_dominant_winner_has_its_margin():
    case = CR.dominant_winner(200, 137)
    for ls in CR.LOGIT_SCALES:
        r, b = CR.case_ref(case, ls, 0)
        assert (r.best == 137).all()
        assert (r.top2_margin > 100.0 * b.final.max(axis=1)).all()


def test_write_back():
    inp = np.arange(12, dtype=np.int32).reshape(3, 4)
    cand = np.array([[50, 51], [60, 61], [70, 71]], np.int32)
    out = CR.write_back(inp, cand, [1, 0, 1], [0, 3, 2])
    want = inp.copy()
    want[0, 0], want[1, 3], want[2, 2] = 51, 60, 71
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(CR.write_back(inp, cand, [0, 0, 0], 1)[:, 1], [50, 60, 70])
    assert inp[0, 0] == 0


def test_bar_functions():
    """monotone in K and in s, the documented values at (K 200, s 100) and (K 1024, s 100), and never below the per-element bars"""
    Ks = [1, 2, 200, 256, 257, 512, 513, 1024]
    for s in (14.3, 100.0):
        v = [CR.clip_rel_bar(K, s) for K in Ks]
        assert all(a <= b for a, b in zip(v, v[1:])) and v[0] < v[-1]
        f = [CR.final_bar_worst(K, s) for K in Ks]
        assert all(a <= b for a, b in zip(f, f[1:]))
    for K in Ks:
        assert CR.clip_rel_bar(K, 14.3) < CR.clip_rel_bar(K, 50.0) < CR.clip_rel_bar(K, 100.0)
        assert CR.final_bar_worst(K, 14.3) < CR.final_bar_worst(K, 100.0)
    assert CR.sum_roundings(200) == 15 and CR.sum_roundings(256) == 15 and CR.sum_roundings(257) == 16 and CR.sum_roundings(1024) == 18
    assert CR.clip_rel_bar(200, 100.0) == pytest.approx(3.67e-5, rel=5e-3)
    assert CR.clip_rel_bar(1024, 100.0) == pytest.approx(3.68e-5, rel=5e-3)
    assert CR.clip_rel_bar(200, float(np.exp(2.6592))) == pytest.approx(6.0e-6, rel=2e-2)
    assert CR.final_bar_worst(200, 100.0) == pytest.approx(7.36e-5, rel=5e-3)
    assert CR.final_bar_worst(1024, 100.0) == pytest.approx(7.39e-5, rel=5e-3)
    # the per-element bars of generated cases stay below the worst case of their shape
    for K in (2, 200, 1024):
        for ls in CR.LOGIT_SCALES:
            for span in (False, True):
                r, b = CR.case_ref(CR.cos_case(K, 0, span=span), ls, 0)
                assert (b.clip_score <= CR.clip_rel_bar(K, r.scale) * r.clip_score + CR.FLOOR * (1 + 1e-9)).all()
                assert (b.final <= CR.final_bar_worst(K, r.scale)).all()
                assert (b.clip_ref <= 2 * 2.0 ** -23).all()


def test_underflowing_tail_gets_the_floor():
    r, b = CR.case_ref(CR.cos_case(64, 0, span=True), CR.LOGIT_SCALES[1], 0)
    tail = r.clip_score < 2.0 ** -126
    assert tail.any()                                   # exp(-200) is far below the smallest normal fp32
    assert (b.clip_score[tail] >= r.clip_score[tail]).all()   # a zero read back there is inside the bar
    assert (b.clip_score[~tail] < 1e-4 * r.clip_score[~tail] + 2 * CR.FLOOR).all()
