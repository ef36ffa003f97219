"""CPU checks of tests/refine_ref.py: the reference's own soundness (the margin gate against brute-force corner assignments, the
plans against their defining properties) and, for exactly the arrays tests/test_refine_kernels_gpu.py feeds the kernels, the
conditions its comparisons rest on (share of gate rows inside the band, mix of gate outcomes, distance of every clip_score to its
row's threshold, share of combine rows left out of the winner comparison, distance of the guard to every deviation)."""
import numpy as np
import pytest

import refine_ref as R


# ---- scan / plans ---------------------------------------------------------------------------------------------------------------------
def test_scan_inputs_have_runs_of_zeros_and_a_loaded_tail():
    for n in R.SCAN_N:
        v = R.scan_lengths(n)
        assert v.size == n and v.min() >= 0 and v.max() <= R.CLIP_LEN
        off, tot, mx = R.scan(v)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(v)])) and tot == v.sum() and mx == v.max()
        if n > 64:
            assert (v == 0).sum() > n // 64 and v[-1] > 0


@pytest.mark.parametrize("K", R.PLAN_K)
@pytest.mark.parametrize("B", R.PLAN_B)
def test_prefix_plan_reference_properties(B, K):
    """The plan encodes every sentence exactly once: trunk + branch rows of a candidate (its representative's, when it is a
    duplicate) are its ids, and the EOS row is the last of them."""
    ids, length = R.plan_rows(B, K)
    assert length.min() >= 2 and length.max() <= R.CLIP_LEN
    for share in (0, 1):
        for dedup in (0, 1):
            pl = R.prefix_plan(ids, length, share, dedup)
            S = B + B * K
            # rebuild the packed id rows the tower would embed: segment s holds ids[src[s], pos0[s] .. pos0[s] + own_len[s])
            rows = {}
            for s in range(S):
                b_, k_ = divmod(int(pl["seg_src"][s]), K)
                for i in range(int(pl["own_len"][s])):
                    rows[int(pl["own_off"][s]) + i] = int(ids[b_, k_, int(pl["seg_pos0"][s]) + i])
            assert len(rows) == pl["totals"][0] == pl["own_off"][S]
            for b in range(B):
                for k in range(K):
                    s = B + b * K + k
                    sr = B + b * K + (int(pl["rep"][b * K + k]) if dedup else k)
                    seen = [rows[int(pl["pre_off"][s]) + i] for i in range(int(pl["pre_len"][s]))]
                    seen += [rows[int(pl["own_off"][sr]) + i] for i in range(int(pl["own_len"][sr]))]
                    assert seen == ids[b, k, :length[b, k]].tolist(), (b, k)
                    assert pl["eos_idx"][b * K + k] == pl["own_off"][sr] + pl["own_len"][sr] - 1
                    assert pl["own_len"][sr] >= 1
                    if dedup:
                        r = int(pl["rep"][b * K + k])
                        assert r <= k and pl["rep"][b * K + r] == r
            if dedup and K >= 6:
                assert pl["totals"][5] >= 2 * B      # the planted duplicates are found
            if dedup and K > 300:
                assert pl["rep"][300] == 260 and pl["rep"][K - 1] == 260 and pl["rep"][257] == 0 and pl["rep"][511] == 0
            if dedup and B > 1:
                assert (pl["rep"][(B - 1) * K:] == 0).all()


def test_prefix_plan_inputs_hit_the_edges():
    ids, length = R.plan_rows(1, 1024)
    pl = R.prefix_plan(ids, length, 1, 1)
    assert 2 in length and R.CLIP_LEN in length
    assert np.array_equal(ids[0, 1, :length[0, 1]], ids[0, 0, :length[0, 1]]) and length[0, 1] < length[0, 0]
    assert np.array_equal(ids[0, 2, :length[0, 0]], ids[0, 0, :length[0, 0]]) and length[0, 2] > length[0, 0]
    assert pl["rep"][4] == 3 and pl["rep"][5] == 3                      # duplicates of a candidate that is not candidate 0
    assert length[0, 7] == length[0, 6] + 1 and pl["rep"][7] == 7       # same ids, another length
    assert pl["own_len"][0] <= 1                                        # the length-2 candidate caps the prefix at len - 1


@pytest.mark.parametrize("K", R.RPLAN_K)
@pytest.mark.parametrize("pattern", R.RPLAN_PATTERNS)
def test_refine_plan_reference_properties(K, pattern):
    clen, trunk, lst, count = R.rplan_inputs(K, pattern)
    B = clen.shape[0]
    assert (trunk[:, None] < clen).all()
    pl = R.refine_plan(clen, trunk, lst, count)
    R_, Kr = pl["R"], pl["Kr"]
    assert R_ == count.sum() and Kr == count.max()
    if pattern == "zero":
        assert R_ == 0 and Kr == 0 and pl["totals"][0] == 0
    if pattern == "one_zero":
        assert pl["own_len"][1] == 0                                    # pb = 0 for the image without a chosen candidate
    flat = [b * K + int(lst[b, i]) for b in range(B) for i in range(count[b])]
    assert pl["rlist"][:R_] == flat and all(v is None for v in pl["rlist"][R_:])
    for r, fl in enumerate(flat):
        b = fl // K
        s = [s for s in range(B, B + B * Kr) if pl["seg_src"][s] == fl and pl["own_len"][s] > 0]
        assert len(s) == 1
        assert pl["eos_idx"][r] == pl["own_off"][s[0]] + clen.reshape(-1)[fl] - trunk[b] - 1
    assert all(v == 0 for v in pl["own_len"][B + B * Kr:])


# ---- selection ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", R.SEL_K)
def test_selection_inputs_and_reference(K):
    p, f = R.sel_inputs(K)
    th = R.sel_theta(K)
    thetas = [th] + [R.theta_of_row(R.SEL_THETA_BASE, R.SEL_SCALE, b) for b in R.SEL_BETAS]
    for b in range(R.SEL_B):
        for t in (thetas[0], thetas[1 + b]):
            assert R.ulp_distance(p[b], t).min() > 4
    pp, _ = R.sel_inputs(K, planted=True)
    u = R.ulp_distance(pp[4], th)
    assert (u == 0).sum() == 1 and (u[u > 0] > 4).all()
    for m in R.sel_m_samples(K):
        kinds = [R.select_row(p[b], f[b], th, m) for b in range(R.SEL_B)]
        for b in range(R.SEL_B):
            R.check_selection_properties(kinds[b], p[b], th, m)
        assert (kinds[0] == 1).all()                                    # no rest: tot = 0, no sample
        if K > 3 and m >= 24:
            assert (kinds[1][70] & 3) == 2 and (kinds[1][70] >> 2) >= 3   # one candidate, several strata
        if K > 3:
            assert kinds[2][5] == 1 and kinds[2][9] == 1                # the first two of the three tied best scores ...
            assert (kinds[2][170] == 1) == bool(p[2][170] > th)         # ... and not the third
            assert kinds[3][0] == 1 and kinds[3][1] == 1                # all scores equal: candidates 0 and 1
        kp = R.select_row(pp[4], f[4], th, m, planted=True)
        top2 = set(np.argsort(-f[4].astype(np.float64), kind="stable")[:2].tolist())
        assert (kp[K // 2] == 1) == (K // 2 in top2)                    # p == theta is NOT above it
        assert K <= 3 or K // 2 not in top2
    with pytest.raises(AssertionError):
        R.select_row(np.array([np.nextafter(th, np.float32(1))] * 2, np.float32), f[0][:2], th, 1)


# ---- margin gate ----------------------------------------------------------------------------------------------------------------------
def _gate_rows():
    for K, scale, beta, need_cos in R.gate_cases():
        p, f, h = R.gate_inputs(K, scale, beta)
        for b in range(R.GATE_B):
            yield K, beta, h, p[b], f[b]


def test_gate_inputs_meet_the_conditions():
    verdict = {1: 0, 0: 0, -1: 0}
    hi_only = 0
    for K, scale, beta, _ in R.gate_cases():    # rows the gate refuses take the full selection: no clip_score near the threshold
        p, f, _ = R.gate_inputs(K, scale, beta)
        assert min(R.ulp_distance(p[b], R.theta_of_row(R.SEL_THETA_BASE, scale, beta)).min() for b in range(R.GATE_B)) > 4
    per_row = {1: 0, 0: 0, -1: 0}               # the launch with per-row betas: same rows, every other one under beta / 2
    for K, scale, beta, _ in R.gate_cases():
        p, f, h = R.gate_inputs(K, scale, beta)
        for b, bt in enumerate(R.gate_row_betas(beta)):
            assert R.ulp_distance(p[b], R.theta_of_row(R.SEL_THETA_BASE, scale, bt)).min() > 4
            per_row[R.gate_verdict(p[b], f[b], bt, h)] += 1
    print(f"per-row betas: in band {per_row[0]}, must gate {per_row[1]}, must not gate {per_row[-1]}")
    # (an extra launch of the same rows; the 20 % mix is asserted below on the betas the rows were planted for)
    assert per_row[0] <= 0.02 * sum(per_row.values()) and min(per_row[1], per_row[-1]) >= 0.1 * sum(per_row.values())
    for K, beta, h, p, f in _gate_rows():
        v = R.gate_verdict(p, f, beta, h)
        verdict[v] += 1
        if K == 1:
            assert v == 1                                               # nobody to overturn the only candidate
        else:
            _, lo, hi = R.gate_terms(p, f, beta, h)
            hi_only += lo.max() < -R.gate_band(beta) and hi.max() > R.gate_band(beta)
    n = sum(verdict.values())
    print(f"gate inputs: {n} rows, in band {verdict[0]}, must gate {verdict[1]}, must not gate {verdict[-1]}, "
          f"refused by the 'others up' extreme alone {hi_only}")
    assert verdict[0] <= 0.02 * n
    assert verdict[1] >= 0.2 * n and verdict[-1] >= 0.2 * n
    assert hi_only >= 10


def test_gate_reference_is_sound():
    """Rows the reference lets through keep their winner under 64 random corner assignments of the cosine errors; rows it
    refuses lose it under the assignment it constructed."""
    rng = np.random.default_rng(3)
    for K, beta, h, p, f in _gate_rows():
        v = R.gate_verdict(p, f, beta, h)
        w = R.first_argmax(f)
        if v == 1:
            for _ in range(64):
                e = rng.choice([-h, h], size=K)
                assert int(np.argmax(R.perturbed_scores(p, f, beta, e))) == w
        elif v == -1:
            _, lo, hi = R.gate_terms(p, f, beta, h)
            r = int(np.argmax(np.maximum(lo, hi)))
            e = np.full(K, h if hi[r] >= lo[r] else -h)
            e[w], e[r] = -h, h
            g = R.perturbed_scores(p, f, beta, e)
            assert g[r] > g[w] and int(np.argmax(g)) != w


def test_gate_band_covers_a_float32_evaluation():
    """The float32 evaluation of the same expression stays well inside the band of the float64 one."""
    f32 = np.float32
    worst = 0.0
    for K, beta, h, p, f in _gate_rows():
        if K == 1:
            continue
        w = R.first_argmax(f)
        up, dn, bt = np.exp(f32(h)), np.exp(f32(-h)), f32(beta)
        ew, bw = p[w] * dn, f[w] - bt * p[w]
        er = p * up
        rest = np.maximum(f32(1) - p[w] - p, f32(0))
        db = (f - bt * p) - bw
        d = np.maximum(db + bt * (er - ew) / (ew + er + rest * dn), db + bt * (er - ew) / (ew + er + rest * up))
        d[w] = -np.inf
        assert d.dtype == np.float32
        diff = abs(float(d.max()) - R.gate_worst64(p, f, beta, h))
        worst = max(worst, diff / R.gate_band(beta))
    print(f"float32 evaluation of the gate vs float64: worst difference {worst:.3f} of the band")
    assert worst < 0.5


# ---- combine ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", R.COMB_K)
def test_combine_inputs_meet_the_conditions(K):
    cos_in, rcos, probs, kind, guard = R.comb_inputs(K)
    scale = float(np.exp(R.COMB_LOGIT_SCALE))
    ref = R.combine_refine(cos_in, probs, R.COMB_ALPHA, R.COMB_BETA, scale, kind, rcos, guard)
    assert np.abs(ref["dev"] - float(guard)).min() > 1e-6
    assert 0 < ref["trips"] < R.COMB_B
    assert ref["mu"][3] == 0 and ref["mu"][4] == 0 and ref["dev"][3] == 0 and ref["dev"][4] > 0
    assert (kind[3] == 3).sum() == 1 and ref["best"][3] == np.nonzero(kind[3] == 3)[0][0]
    assert abs(ref["best_cos"][3] - float(cos_in[3, ref["best"][3]])) > 1e-4    # the exact cosine, not the screening one
    # the sample's weights matter: on the hand-made row the unweighted mean lands five tolerances of clip_ref away
    if K > 3:
        k2 = (kind[5] & 3) == 2
        d = cos_in[5].astype(np.float64) - rcos[5].astype(np.float64)
        assert (kind[5][k2] >> 2).tolist() == [1, 2, 7, 14]
        assert abs(d[k2].mean() - ref["mu"][5]) > 1e-5


def test_combine_inputs_leave_few_winners_out():
    gaps = np.concatenate([R.combine_refine(c, p, R.COMB_ALPHA, R.COMB_BETA, float(np.exp(R.COMB_LOGIT_SCALE)), k, r, g)["top2_gap"]
                           for c, r, p, k, g in (R.comb_inputs(K) for K in R.COMB_K)])
    out = int((gaps <= 1e-5).sum())
    print(f"combine inputs: {out} of {gaps.size} rows left out of the winner comparison")
    assert out <= 0.05 * gaps.size


@pytest.mark.parametrize("K", R.COMB_K)
@pytest.mark.parametrize("D", R.COMB_D)
def test_cosine_inputs(K, D):
    feat, img, rlist, n = R.cosine_inputs(K, D)
    assert 0 < n < feat.shape[0] and np.isnan(feat[n:]).all() and (rlist[n:] == -1).all()
    assert np.unique(rlist[:n]).size == n and rlist[:n].max() < img.shape[0] * K
