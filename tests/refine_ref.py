"""NumPy reference of the integer and selection side of the screen-then-refine engine, for tests/: the scan, the shared-prefix
plan with exact de-duplication, the selection of the candidates to re-encode, the margin gate, the plan of the refine pass, the
exact cosines and the refine branch of the final combine -- plus the inputs tests/test_refine_kernels_gpu.py runs the kernels on
(tests/test_refine_ref_cpu.py asserts the conditions the comparisons rest on for these very arrays).

TEST INFRASTRUCTURE: written from the statements of the operations in csrc/kernels.h and the comments of csrc/bridge.hip /
csrc/combine.hip, not from the kernels.  Integer parts are plain Python loops; the stratified sample is formed in float32 in
candidate order as the comment above refine_select_kernel states it (one thread, IEEE adds, one multiply, one divide), the gate,
the cosines and the scores in float64."""
import numpy as np

F32 = np.float32
CLIP_LEN = 77
EPS32 = float(np.finfo(np.float32).eps)


# ---- scan ---------------------------------------------------------------------------------------------------------------------
def scan(length):
    """off [n + 1] = exclusive scan, (sum, max) -- the maximum is never below 0."""
    off = [0]
    mx = 0
    for v in length:
        off.append(off[-1] + int(v))
        mx = max(mx, int(v))
    return np.array(off, np.int64), off[-1], mx


# ---- shared-prefix plan, de-duplication, finish -----------------------------------------------------------------------------------
def prefix_plan(ids, length, share, dedup):
    """ids [B, K, 77], length [B, K] -> dict of the segment tables (S = B + B*K slots: B trunks, then the B*K branches) and the
    eight totals words.  `rep` is None without de-duplication."""
    B, K = length.shape
    S = B + B * K
    own, pre, src, pos0 = ([0] * S for _ in range(4))
    rep = [0] * (B * K) if dedup else None
    img_max = [0] * B
    max_len = max_branch = dups = pairs = 0
    for b in range(B):
        l0 = int(length[b, 0])
        pb = 1 << 30
        mx = 0
        for k in range(K):
            lk = int(length[b, k])
            c = 0
            while c < min(lk, l0) and ids[b, k, c] == ids[b, 0, c]:
                c += 1
            pb = min(pb, c, lk - 1)     # the common prefix never swallows a candidate's last (EOS) row
            mx = max(mx, lk)
        if not share:
            pb = 0
        own[b], pre[b], src[b], pos0[b] = pb, 0, b * K, 0
        img_max[b] = mx - pb
        max_len, max_branch = max(max_len, mx), max(max_branch, mx - pb)
        pairs += pb * (pb + 1) // 2
        seen = {}
        for k in range(K):
            s = B + b * K + k
            lk = int(length[b, k])
            o = lk - pb
            if dedup:
                key = (lk, ids[b, k, :lk].tobytes())
                r = seen.setdefault(key, k)     # the lowest identical candidate
                rep[b * K + k] = r
                if r != k:
                    o = 0
                    dups += 1
            own[s], pre[s], src[s], pos0[s] = o, pb, b * K + k, pb
            pairs += o * pb + o * (o + 1) // 2
    own_off, rows, longest = scan(own)
    pre_off = [0] * S
    eos = [0] * (B * K)
    for i in range(B * K):
        b = i // K
        pre_off[B + i] = int(own_off[b])
        sr = B + b * K + rep[i] if dedup else B + i
        eos[i] = int(own_off[sr]) + own[sr] - 1
    totals = [rows, longest, 0, max_len, max_branch, dups, int(own_off[B]), pairs]
    out = dict(own_len=own, pre_len=pre, seg_src=src, seg_pos0=pos0, own_off=own_off, pre_off=pre_off, eos_idx=eos,
               img_max=img_max, totals=totals)
    out = {k: np.asarray(v, np.int64) for k, v in out.items()}
    out["rep"] = None if rep is None else np.asarray(rep, np.int64)
    return out


# ---- plan of the refine pass --------------------------------------------------------------------------------------------------------
def refine_plan(clip_len, trunk_len, lst, count):
    """clip_len, lst [B, K], trunk_len, count [B] -> the tables of the regular B x Kr plan (entries beyond what the plan defines are
    None: the kernels leave them alone) and the sixteen totals words."""
    B, K = clip_len.shape
    S = B + B * K
    count_off, R, Kr = scan(count)
    own = [0] * S                       # the engine's memset: empty and unused slots read 0
    pre, src, pos0, pre_off = ([None] * S for _ in range(4))
    rlist, eos = [None] * (B * K), [None] * (B * K)
    img_max = [0] * B
    max_len = max_branch = pairs = 0
    for b in range(B):
        n = int(count[b])
        pb = int(trunk_len[b]) if n > 0 else 0
        own[b], pre[b], src[b], pos0[b] = pb, 0, b * K, 0
        if n > 0:
            pairs += pb * (pb + 1) // 2
        for i in range(Kr):
            s = B + b * Kr + i
            if i >= n:                  # empty slot: a zero-length segment of this image's trunk
                pre[s], src[s], pos0[s] = pb, b * K, pb
                continue
            flat = b * K + int(lst[b, i])
            ln = int(clip_len.reshape(-1)[flat])
            own[s], pre[s], src[s], pos0[s] = ln - pb, pb, flat, pb
            rlist[int(count_off[b]) + i] = flat
            img_max[b] = max(img_max[b], ln - pb)
            max_len, max_branch = max(max_len, ln), max(max_branch, ln - pb)
            pairs += (ln - pb) * pb + (ln - pb) * (ln - pb + 1) // 2
    own_off, rows, longest = scan(own)
    for b in range(B):
        pre_off[b] = 0
        for i in range(Kr):
            s = B + b * Kr + i
            pre_off[s] = int(own_off[b])
            if i < int(count[b]):
                eos[int(count_off[b]) + i] = int(own_off[s]) + own[s] - 1
    totals = [rows, longest, 0, max_len, max_branch, 0, 0, pairs, R, Kr] + [0] * 6
    return dict(count_off=count_off, own_len=own, pre_len=pre, seg_src=src, seg_pos0=pos0, own_off=own_off, pre_off=pre_off,
                rlist=rlist, eos_idx=eos, img_max=img_max, totals=totals, R=R, Kr=Kr)


# ---- selection ----------------------------------------------------------------------------------------------------------------------
def theta_of_row(theta_base, scale, beta):
    """the per-row mass threshold, float32: theta_base / max(beta * scale, 1e-6)"""
    return F32(theta_base) / max(F32(beta) * F32(scale), F32(1e-6))


def ulp_distance(p, theta):
    """|p - theta| in units of theta's float32 spacing"""
    return np.abs(np.asarray(p, np.float64) - float(theta)) / float(np.spacing(F32(theta)))


def first_argmax(f):
    """first index of the largest non-NaN value (0 when there is none)"""
    f = np.asarray(f)
    ok = ~np.isnan(f)
    if not ok.any():
        return 0
    return int(np.argmax(np.where(ok, f, -np.inf)))


def select_row(p, f, theta, m_samples, planted=False):
    """kind [K] of one image that takes the full selection.  Asserts the condition the exact comparison rests on: no p within
    4 ulp of theta (`planted`: values EQUAL to theta are allowed -- the scalar form takes theta as an input, so equality is
    decided without arithmetic)."""
    p = np.asarray(p, F32)
    K = p.size
    u = ulp_distance(p, theta)
    near = (u <= 4) & ~((u == 0) & planted)
    assert not near.any(), ("a clip_score within 4 ulp of theta", p[near], theta)
    kind = [1 if p[k] > F32(theta) else 0 for k in range(K)]
    g = np.array(f, np.float64)
    for _ in range(2):                  # the first argmax of the fused score, then the first runner-up
        w = first_argmax(g)
        kind[w] = 1
        g[w] = -np.inf
    tot = F32(0)
    for k in range(K):
        if not kind[k]:
            tot = F32(tot + p[k])
    if m_samples > 0 and tot > 0:
        cum = F32(0)
        j = 0
        mf = F32(m_samples)
        for k in range(K):
            if j >= m_samples:
                break
            if kind[k]:
                continue
            cum = F32(cum + p[k])
            hits = 0
            while j < m_samples and cum >= F32(F32(F32(j) + F32(0.5)) * tot) / mf:
                hits += 1
                j += 1
            if hits:
                kind[k] = 2 | (hits << 2)
    return np.array(kind, np.int64)


def check_selection_properties(kind, p, theta, m_samples, lst=None, count=None):
    """what holds of a full selection whatever the arithmetic"""
    kind = np.asarray(kind)
    k2 = (kind & 3) == 2
    rest = (kind & 3) != 1
    if m_samples > 0 and float(np.asarray(p, np.float64)[rest].sum()) > 0:
        assert int((kind[k2] >> 2).sum()) == m_samples, ("strata", int((kind[k2] >> 2).sum()), m_samples)
    else:
        assert not k2.any()
    assert not (np.asarray(p, F32)[k2] > F32(theta)).any()
    assert ((kind[~k2] == 0) | (kind[~k2] == 1)).all()
    if lst is not None:
        nz = np.nonzero(kind)[0]
        assert count == nz.size and np.array_equal(np.asarray(lst)[:count], nz)


# ---- margin gate ----------------------------------------------------------------------------------------------------------------------
def gate_band(beta):
    """evaluation error of the gate's handful of float32 operations on values of size <= beta"""
    return 32.0 * EPS32 * max(1.0, float(beta))


def gate_terms(p, f, beta, h):
    """float64, from the float32 scores: winner w (first argmax of f) and, per challenger r, f_r - f_w under the two extreme
    assignments (w's logit down by h, r's up by h, every other one down / up by h) -> (w, d_lo [K], d_hi [K]); entry w is -inf."""
    p = np.asarray(p, np.float64)
    f = np.asarray(f, np.float64)
    w = first_argmax(f)
    K = p.size
    base = f - beta * p
    up, dn = np.exp(h), np.exp(-h)
    d = np.full((2, K), -np.inf)
    tot = p.sum()
    for r in range(K):
        if r == w:
            continue
        ew, er = p[w] * dn, p[r] * up
        rest = max(tot - p[w] - p[r], 0.0)
        for i, x in enumerate((dn, up)):
            d[i, r] = (base[r] + beta * er / (ew + er + rest * x)) - (base[w] + beta * ew / (ew + er + rest * x))
    return w, d[0], d[1]


def gate_worst64(p, f, beta, h):
    if np.isnan(np.asarray(f)).any():
        return np.inf                   # a NaN score never passes the gate
    _, lo, hi = gate_terms(p, f, beta, h)
    return float(max(lo.max(), hi.max()))


def gate_verdict(p, f, beta, h):
    """+1 the gate must pass the row, -1 it must not, 0 inside the band (either outcome)"""
    worst = gate_worst64(p, f, beta, h)
    band = gate_band(beta)
    return 1 if worst < -band else -1 if worst > band else 0


def perturbed_scores(p, f, beta, e):
    """float64 fused scores when candidate k's logit moves by e[k]"""
    p = np.asarray(p, np.float64)
    f = np.asarray(f, np.float64)
    q = p * np.exp(e)
    return (f - beta * p) + beta * q / q.sum()


def gated_row(K, w, need_cos):
    kind = np.zeros(K, np.int64)
    if need_cos:
        kind[w] = 3
    return kind


# ---- exact cosines / the refine branch of the final combine -----------------------------------------------------------------------
def cosines(feat, img, rows_img):
    """feat [R, D] float32 rows against img [B, D] (row r belongs to image rows_img[r]), float64"""
    t = np.asarray(feat, np.float64)
    i = np.asarray(img, np.float64)
    t = t / np.linalg.norm(t, axis=1, keepdims=True)
    i = i / np.linalg.norm(i, axis=1, keepdims=True)
    return np.einsum("rd,rd->r", t, i[np.asarray(rows_img)])


def combine_refine(cos_in, probs, alpha, beta, scale, kind, rcos, guard):
    """float64: dict(clip_score, clip_ref, final [B, K], best, best_cos, mu, dev [B], top2_gap [B], max_dev, trips)."""
    cos_in = np.asarray(cos_in, np.float64)
    rc = np.asarray(rcos, np.float64)
    kind = np.asarray(kind)
    B, K = cos_in.shape
    kd = kind & 3
    exact = (kd == 1) | (kd == 2)
    wgt = np.where(kd == 2, kind >> 2, 0).astype(np.float64)
    d = np.where(exact, cos_in - np.where(exact, rc, 0.0), 0.0)
    mu = np.array([(wgt[b] * d[b]).sum() / wgt[b].sum() if wgt[b].sum() > 0 else 0.0 for b in range(B)])
    dev = np.array([np.abs(d[b] - mu[b])[exact[b]].max() if exact[b].any() else 0.0 for b in range(B)])
    ce = np.where(exact, np.where(exact, rc, 0.0), cos_in - mu[:, None])
    lg = ce * scale
    cs = np.exp(lg - lg.max(axis=1, keepdims=True))
    cs /= cs.sum(axis=1, keepdims=True)
    fin = alpha * np.asarray(probs, np.float64) + beta * cs
    best = fin.argmax(axis=1)
    bcos = np.array([rc[b, best[b]] if kd[b, best[b]] == 3 else ce[b, best[b]] for b in range(B)])
    srt = np.sort(fin, axis=1)
    gap = srt[:, -1] - srt[:, -2] if K > 1 else np.full(B, np.inf)
    return dict(clip_score=cs, clip_ref=ce, final=fin, best=best, best_cos=bcos, mu=mu, dev=dev, top2_gap=gap,
                max_dev=float(dev.max()), trips=int((dev > guard).sum()))


# =====================================================================================================================================
# The inputs of tests/test_refine_kernels_gpu.py.  Everything below is deterministic; tests/test_refine_ref_cpu.py asserts on these
# arrays the conditions the GPU comparisons rest on.
# =====================================================================================================================================
SCAN_N = (1, 2, 1023, 1024, 1025, 2047, 2049, 5 * 1024 + 5, 70001)


def scan_lengths(n):
    """lengths in 0..77 with runs of zeros (de-duplicated candidates, empty refine slots)"""
    rng = np.random.default_rng(n)
    v = rng.integers(0, CLIP_LEN + 1, size=n)
    for s in rng.integers(0, n, size=max(1, n // 64)):
        v[s:s + int(rng.integers(1, 40))] = 0
    if n > 2:
        v[n - 1] = CLIP_LEN             # the last slot carries rows, so a dropped tail shows in every total
    return v.astype(np.int32)


PLAN_B = (1, 3)
PLAN_K = (1, 2, 255, 256, 257, 1024)


def plan_rows(B, K, seed=0):
    """ids [B, K, 77], length [B, K]: per image a common prefix, random tails, and the planted relations among candidates (each
    wherever K has room): all-identical image (the last one when B > 1), candidates equal to candidate 0 up to their own EOS but
    shorter / longer, duplicates of a candidate other than 0, duplicates that first appear beyond index 255, same ids under
    another length, length 2 and length 77.  The ids behind a row's length are noise the kernels must not read."""
    rng = np.random.default_rng(100 * K + B + seed)
    ids = rng.integers(1000, 40000, size=(B, K, CLIP_LEN)).astype(np.int32)
    length = np.zeros((B, K), np.int32)
    for b in range(B):
        pfx = int(rng.integers(1, 9))
        l0 = int(rng.integers(pfx + 6, 40))
        ids[b, :, 0] = 49406
        ids[b, :, 1:pfx] = ids[b, 0, 1:pfx]
        for k in range(K):
            length[b, k] = l0 if k == 0 else int(rng.integers(pfx + 2, 60))
        free = list(range(1, K))

        def take():
            return free.pop(0) if free else None
        k = take()
        if k is not None:               # candidate 0 cut short: equal to it up to its own last row
            length[b, k] = l0 - 3
            ids[b, k, :l0 - 3] = ids[b, 0, :l0 - 3]
        k = take()
        if k is not None:               # candidate 0 and more: equal over all of candidate 0's rows
            length[b, k] = l0 + 4
            ids[b, k, :l0] = ids[b, 0, :l0]
        a, d1, d2 = take(), take(), take()
        if d2 is not None:              # duplicates of a candidate that is not candidate 0
            for d in (d1, d2):
                length[b, d] = length[b, a]
                ids[b, d, :length[b, a]] = ids[b, a, :length[b, a]]
        a, d1 = take(), take()
        if d1 is not None:              # same ids, another length: not a duplicate
            length[b, d1] = length[b, a] + 1
            ids[b, d1, :length[b, a] + 1] = ids[b, a, :length[b, a] + 1]
        k = take()
        if k is not None:
            length[b, k] = 2
        k = take()
        if k is not None:
            length[b, k] = CLIP_LEN
        if K > 300:                     # duplicates whose first occurrence lies beyond index 255, and of candidate 0 out there
            for a, ds in ((260, (300, K - 1)), (0, (257, 511))):
                for d in ds:
                    length[b, d] = length[b, a]
                    ids[b, d, :length[b, a]] = ids[b, a, :length[b, a]]
        elif K > 256:
            length[b, 256] = length[b, 200]
            ids[b, 256, :length[b, 200]] = ids[b, 200, :length[b, 200]]
        if K >= 200:                    # the tail of the K candidates: one sentence (the token mask's [PAD] candidates)
            for d in range(K - 40, K - 1):
                length[b, d] = length[b, K - 45]
                ids[b, d, :length[b, d]] = ids[b, K - 45, :length[b, d]]
    if B > 1:
        length[B - 1, :] = length[B - 1, 0]
        ids[B - 1, :, :] = ids[B - 1, 0, :]
        ids[B - 1, :, length[B - 1, 0]:] = rng.integers(1000, 40000, size=(K, CLIP_LEN - length[B - 1, 0]))
    return ids, length


# ---- selection inputs ---------------------------------------------------------------------------------------------------------------
SEL_K = (1, 2, 3, 200, 256, 257, 1024)
SEL_B = 5
SEL_SCALE = 100.0
SEL_THETA_BASE = 2.0
SEL_BETAS = (2.0, 1.0, 0.5, 2.0, 1.5)       # per row, the _rows / _draw forms
SEL_TAUS = (0.0, 0.7, 0.0, 0.0, 0.3)        # the _draw forms: rows 1 and 4 draw


def sel_m_samples(K):
    return (0, 1, 24, K + 5)


def sel_theta(K):
    """the scalar form's threshold: above the rest of every planted row, below row 0's near-uniform masses"""
    return F32(0.5 / K) if K > 3 else F32(0.2)


def sel_inputs(K, planted=False):
    """clip_score, final_score [5, K] float32 for the selection proper (no gate):
    row 0 every candidate above sel_theta(K) (no rest, tot = 0); row 1 a few heavy candidates, ONE candidate just below theta that
    holds most of the rest's mass (it stands for several strata) and dust; row 2 the best fused score shared by three
    candidates; row 3 all fused scores equal; row 4 a softmax at scale 100 (`planted`: one clip_score EQUAL to theta)."""
    rng = np.random.default_rng(7000 + K)
    th = float(sel_theta(K))
    p = np.zeros((SEL_B, K))
    f = np.zeros((SEL_B, K))
    p[0] = (1.0 + 0.2 * rng.uniform(-1, 1, K)) / K if K > 3 else (0.3 + 0.05 * rng.uniform(0, 1, K))
    f[0] = rng.uniform(0, 1, K)
    dust = rng.uniform(1e-7, 1e-6, K)
    p[1] = dust
    if K > 3:
        p[1, [3, 50, K - 2]] = (0.5, 0.3, 0.19)
        p[1, 70] = 0.9 * th
        p[1, 120] = 0.3 * th
    else:
        p[1, 0] = 0.9 * th
    f[1] = 0.1 * rng.uniform(0, 1, K) + 2.0 * p[1]
    lg = rng.standard_normal(K) * 5.0
    sm = np.exp(lg - lg.max())
    p[2] = sm / sm.sum()
    f[2] = rng.uniform(0, 0.5, K)
    f[2, [i % K for i in (5, 9, 170)]] = 0.75
    lg = rng.standard_normal(K) * 5.0
    sm = np.exp(lg - lg.max())
    p[3] = sm / sm.sum()
    f[3] = 0.25
    lg = rng.standard_normal(K) * 5.0
    sm = np.exp(lg - lg.max())
    p[4] = sm / sm.sum()
    f[4] = 0.02 * rng.dirichlet(np.ones(K)) + 2.0 * p[4]
    p = p.astype(F32)
    if planted:
        p[4, K // 2] = F32(th)
    return p, f.astype(F32)


# ---- gate inputs ----------------------------------------------------------------------------------------------------------------------
GATE_K = (1, 2, 3, 64, 200, 257, 1024)
GATE_SCALES = (20.0, 100.0)
GATE_B = 32
GATE_DELTA = 7e-4


def gate_cases():
    """(K, scale, beta, need_cos) of every gate launch"""
    out = []
    for i, K in enumerate(GATE_K):
        for j, scale in enumerate(GATE_SCALES):
            out.append((K, scale, (0.5, 1.0, 2.0)[(i + j) % 3], (i + j) & 1))
    return out


def gate_inputs(K, scale, beta):
    """clip_score (a float32 softmax at `scale`), final_score [GATE_B, K] float32 and h = GATE_DELTA * scale.  Rows 0, 3, 6, ...
    keep their random scores; the others get a planted runner-up whose worst-case margin sits close to 0 on either side:
    rows 1 mod 3 just not gateable, rows 2 mod 3 alternately just gateable and caught by the 'others up' extreme alone."""
    rng = np.random.default_rng(int(31 * K + scale))
    h = GATE_DELTA * scale
    cos = 0.22 + 0.04 * rng.standard_normal((GATE_B, K))
    lg = cos * scale
    sm = np.exp(lg - lg.max(axis=1, keepdims=True))
    p = (sm / sm.sum(axis=1, keepdims=True)).astype(F32)
    pr = rng.dirichlet(np.ones(K) * 0.3, size=GATE_B)
    f = (0.1 * pr + beta * p.astype(np.float64)).astype(F32)
    if K == 1:
        return p, f, h
    band = gate_band(beta)
    for b in range(GATE_B):
        mode = b % 3
        if mode == 0:
            continue
        w, lo, hi = gate_terms(p[b], f[b], beta, h)
        g = np.array(f[b], np.float64)
        g[w] = -np.inf
        r = int(np.argmax(g))           # the runner-up moves
        d_r = max(lo[r], hi[r])
        shift = d_r - (float(f[b, r]) - float(f[b, w]))     # what the adversarial errors add to f_r - f_w
        if mode == 1:
            target = 0.3 * shift
        elif (b // 3) % 2 == 0:
            target = -0.3 * shift
        else:                           # between the two extremes: d_lo < 0 < d_hi (or the reverse)
            target = 0.5 * abs(hi[r] - lo[r])
        if abs(target) < 8 * band or target >= shift:
            continue
        f[b, r] = F32(float(f[b, w]) + target - shift)
    return p, f, h


def gate_row_betas(beta):
    """the per-row launch of a gate case: every other row under half the case's beta"""
    return [beta if b % 2 == 0 else 0.5 * beta for b in range(GATE_B)]


# ---- refine-plan inputs ---------------------------------------------------------------------------------------------------------------
RPLAN_K = (3, 200, 1024)
RPLAN_PATTERNS = ("zero", "one_zero", "full", "uneven", "selection")


def rplan_inputs(K, pattern):
    """clip_len, lst [B, K], trunk_len, count [B]; the entries of lst behind count[b] are noise"""
    rng = np.random.default_rng(900 + K)
    B = 4
    trunk = rng.integers(0, 9, size=B).astype(np.int32)
    trunk[1] = 0
    clen = np.stack([rng.integers(t + 1, CLIP_LEN + 1, size=K) for t in trunk]).astype(np.int32)
    clen[0, 0], clen[2, K - 1] = CLIP_LEN, trunk[2] + 1
    lst = np.full((B, K), -7, np.int32)
    if pattern == "zero":
        count = np.zeros(B, np.int32)
    elif pattern == "one_zero":
        count = np.array([min(K, 5), 0, min(K, 17), 1], np.int32)
    elif pattern == "full":
        count = np.full(B, K, np.int32)
    elif pattern == "uneven":
        count = np.array([1, K, 0, min(K, 2)], np.int32)
    else:                               # what the selection reference chooses on the selection inputs
        p, f = sel_inputs(K)
        kinds = [select_row(p[b], f[b], sel_theta(K), 24) for b in (1, 2, 3, 4)]
        count = np.array([np.count_nonzero(k) for k in kinds], np.int32)
        for b, k in enumerate(kinds):
            lst[b, :count[b]] = np.nonzero(k)[0]
        return clen, trunk, lst, count
    for b in range(B):
        lst[b, :count[b]] = np.sort(rng.choice(K, size=count[b], replace=False))
    return clen, trunk, lst, count


# ---- cosine / combine inputs ----------------------------------------------------------------------------------------------------------
COMB_K = (3, 200, 1024)
COMB_D = (64, 512)
COMB_B = 6
COMB_LOGIT_SCALE = float(np.log(100.0))
COMB_ALPHA, COMB_BETA = 0.02, 2.0


def comb_inputs(K):
    """cos_in (screening cosines), rcos (exact cosines where marked, NaN elsewhere: never read), probs, kind [6, K], guard.
    Rows 0-2: the selection reference at 24 strata on the row's own screening scores; row 3: a margin-gated image (kind 3 on
    its winner); row 4: mass carriers only (no sample, mu = 0); row 5: a hand-made sample with unequal weights.  The errors of
    the sampled candidates grow with their weight, so that an unweighted mean lands elsewhere."""
    rng = np.random.default_rng(4000 + K)
    B = COMB_B
    scale = float(np.exp(COMB_LOGIT_SCALE))
    cos_in = (0.22 + 0.04 * rng.standard_normal((B, K))).astype(F32)
    lg = cos_in.astype(np.float64) * scale
    sm = np.exp(lg - lg.max(axis=1, keepdims=True))
    p = (sm / sm.sum(axis=1, keepdims=True)).astype(F32)
    probs = rng.dirichlet(np.ones(K) * 0.3, size=B).astype(F32)
    f = (COMB_ALPHA * probs.astype(np.float64) + COMB_BETA * p.astype(np.float64)).astype(F32)
    theta = theta_of_row(SEL_THETA_BASE, scale, COMB_BETA)
    kind = np.zeros((B, K), np.int64)
    for b in range(3):
        kind[b] = select_row(p[b], f[b], theta, 24)
    kind[3, first_argmax(f[3])] = 3
    kind[4] = select_row(p[4], f[4], theta, 0)
    kind[5] = select_row(p[5], f[5], theta, 0)
    free = np.nonzero(kind[5] == 0)[0]
    err = 3e-4 + 1e-4 * rng.standard_normal((B, K))
    for i, (k, hits) in enumerate(zip(free[:4], (1, 2, 7, 14))):
        kind[5, k] = 2 | (hits << 2)
        err[5, k] = 1e-4 + 4e-5 * hits
    err += np.where((kind & 3) == 2, 4e-5 * ((kind >> 2) - 1), 0.0)    # the screening error grows with the weight: the mean needs its weights
    marked = kind != 0
    rcos = np.where(marked, cos_in.astype(np.float64) - err, np.nan).astype(F32)
    ref = combine_refine(cos_in, probs, COMB_ALPHA, COMB_BETA, scale, kind, rcos, 0.0)
    dv = np.sort(ref["dev"])
    i = int(np.argmax(np.diff(dv)))     # the guard sits in the widest gap between two images' deviations
    guard = F32(0.5 * (dv[i] + dv[i + 1]))
    return cos_in, rcos, probs, kind, guard


def cosine_inputs(K, D):
    """feat [n_rows_max, D] (rows behind n_rows: NaN, never read), img [B, D], rlist [n_rows_max] (behind n_rows: -1), n_rows, from
    the refine plan of the selection pattern"""
    rng = np.random.default_rng(5000 + K + D)
    clen, trunk, lst, count = rplan_inputs(K, "selection")
    plan = refine_plan(clen, trunk, lst, count)
    R = plan["R"]
    n_max = R + 7
    feat = np.full((n_max, D), np.nan, F32)
    feat[:R] = rng.standard_normal((R, D)).astype(F32) * 3.0
    img = rng.standard_normal((clen.shape[0], D)).astype(F32)
    rlist = np.full(n_max, -1, np.int32)
    rlist[:R] = plan["rlist"][:R]
    return feat, img, rlist, R
