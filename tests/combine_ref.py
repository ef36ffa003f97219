"""NumPy float64 reference of the score-combine kernel (conzic_amd/csrc/combine.hip: cosine_kernel and the instantiations of
combine_kernel without rivals), its error bars, and the inputs of tests/test_combine_kernel_gpu.py.  TEST INFRASTRUCTURE: written
from the formulas of the reference project (clip/clip.py:86-98, gen_utils.py:77-80, control_gen_utils.py:59 and :163-169), not from
the kernel; tests/test_combine_ref_cpu.py pins it against the torch formulas of oracle/.

The operation, per row b of K candidates (s = exp(logit_scale)):
    cos_k   = <t_k / |t_k|, i / |i|>                    (or given)
    clip_k  = softmax_K(cos * s)_k,      ref_k = cos_k
    final_k = alpha * probs_k + beta * clip_k
              + gamma * softmax_K(raw)_k + 0.1 * (1 - exp(repeats_k))        control 1 (sentiment)
              + gamma * softmax_K(raw / 0.1)_k                                control 2 (POS)
    best    = first argmax_K(final);   inp[b, col_b] = cand[b, best]

THE BARS.  Derived from the number format and the order of operations the formulas fix, not from what the kernel returns.
u = 2^-24 (the unit roundoff of fp32: one rounding moves a value by at most u relative); an elementary function (expf, the
division) is allowed one ulp = 2u relative, the project's figure (tests/gemm_range.py, the activation derivation).  All bounds are
first order in u; the second-order terms are below 1e-13 relative and the exponent error goes through expm1, not through its
linearisation.

(a) a softmax over K of logits v_k that the kernel holds with an absolute error of at most e_k each (softmax_bar):
    the kernel forms  exp(v_k - m) / sum_j exp(v_j - m)  with m the largest computed logit.  Subtracting the SAME m in the numerator
    and in every term of the sum changes nothing (softmax is shift invariant), so the error of m itself cancels: this holds
    whether or not the compiler contracts  c * s - m  into one FMA, in either loop.  What is left in the exponent of term k is
        E_k = e_k + u |x_k|,   x_k = v_k - max v      (the logit's own error, and the rounding of the difference)
    and the softmax moves by at most the relative amount  E_k + sum_j p_j E_j  (numerator, and the p-weighted mean over the sum's
    terms), i.e. by  expm1(E_k + sum_j p_j E_j).  On top, relative roundings counted in u:
        2 (expf, numerator) + 2 (expf, terms of the sum: a weighted mean of errors <= 2u) + 2 (the division)
        + ceil(K / 256) - 1 (a thread's strided partial sum) + 6 (the butterfly over a 64-lane wave) + 3 (the four waves)
      = ceil(K / 256) + 14,   taken as gamma_n = n u / (1 - n u).
    Absolute floor 2^-126: the sum is >= 1 (its largest term is exp(0)), so a softmax value below the smallest normal fp32 comes
    from an expf result in the subnormal range, which the hardware may flush to zero or round to a subnormal: up to 2^-126 absolute
    whatever the relative bound says.  With cosines spanning [-1, 1] at s = 100 the tail is exp(-200) ~ 1e-87 and reads back as 0.
(b) clip_score, cosine-input mode: v = c * s with c an fp32 input and s the fp32 scale the kernel is handed (expf(logit_scale), formed
    on the host once per checkpoint; the hook returns it and the reference takes that number as exact: against exp(logit_scale) in
    float64 it is off by up to 2u relative, which alone moves exp(x) at x = -80 by 160u and would have to be added to every bar
    below), so e_k = u s |c_k| (one product).  Worst case over |c| <= 1:
    |x| <= 2 s, E <= 3 u s per side, 6 u s in all = 3.58e-5 at s = 100 (5.1e-6 at s = 14.3).  With the sum term
    (clip_rel_bar):  K 200, s 100: 3.67e-5;  K 1024, s 100: 3.68e-5 -- relative to clip_k.  The tests use the per-element value
    from the actual cosines (uniform in +-0.4: about 0.4 of the worst case).
(c) clip_ref = (c * s) / s: the product's rounding and the division's: within 2 ulp of the input cosine (REF_ULPS).
(d) the control softmax: sentiment raw scores are fp32 inputs divided by 1.0 (exact): e_k = 0.  POS: raw / 0.1f -- the constant is
    fp32(0.1) (u relative) and the division is allowed its ulp (2u): e_k = 3 u |v_k|, v = raw / 0.1.
(e) final: every product and every sum rounds once (u of its own value) -- with contraction on, an FMA skips the product's
    rounding; the bound allows for two roundings everywhere, so it holds either way:
        |beta| * bar(clip) + u (|alpha p| + |beta clip| + |alpha p + beta clip|)
      + |gamma| * bar(sp) + u (|gamma sp| + |partial sum|)                                              control 1, 2
      + 0.1 (2u e^r + u |1 - e^r|) + 2u |0.1 (1 - e^r)| + u |final|                                     control 1
    (expf's ulp, the rounding of 1 - e^r; fp32(0.1) and the product; the last sum).  alpha, beta, gamma enter as the fp32 values
    the record holds.  Worst case without control at alpha 0.02, beta 2 and p, clip <= 1 (final_bar_worst): 7.36e-5 at (K 200, s
    100) and 7.39e-5 at (K 1024, s 100), absolute.
(f) feature-input mode keeps the project's bar on an fp32 cosine against fp64: |clip_ref - cos| <= 2e-6 (COS_BAR).  Downstream the
    same derivation with e_k = s * 2e-6 + u s |c_k| in (a).

WINNERS.  best[b] must be the reference's first argmax on every row whose reference top-2 margin exceeds twice the row's largest
final bar; the generators below are seeded so that the reference alone leaves out at most 5 % of a case's rows and keeps at least
one (tests/test_combine_ref_cpu.py asserts it)."""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -126
COS_BAR = 2e-6
REF_ULPS = 2
LOGIT_SCALES = (2.6592, float(np.log(100.0)))
MAX_LEFT_OUT = 0.05


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def softmax(v):
    v = np.asarray(v, dtype=np.float64)
    e = np.exp(v - v.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def cosines(text_feat, img, B):
    t = np.asarray(text_feat, dtype=np.float64).reshape(B, -1, np.asarray(text_feat).shape[-1])
    i = np.asarray(img, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = t / np.linalg.norm(t, axis=2, keepdims=True)
        i = i / np.linalg.norm(i, axis=1, keepdims=True)
    return np.einsum("bkd,bd->bk", t, i)


def _col(x, B):
    return np.broadcast_to(np.asarray(x, dtype=np.float64), (B,))[:, None]


def top2_margin(final):
    """[B]: the gap between the best and the second-best score of every row (inf at K = 1)."""
    f = np.asarray(final, dtype=np.float64)
    if f.shape[1] < 2:
        return np.full(f.shape[0], np.inf)
    top = -np.partition(-f, 1, axis=1)[:, :2]
    return top[:, 0] - top[:, 1]


def combine(cos, logit_scale, probs, alpha, beta, gamma=0.0, control=0, senti_raw=None, repeats=None, scale=None):
    """cos: [B, K] cosines, or a pair (text_feat [B*K, D], img [B, D]).  alpha / beta / gamma / control: scalars or [B].
    scale: the fp32 number expf(logit_scale) the kernel was handed (the hook returns it), taken as exact in place of
    exp(logit_scale): the scale is formed on the host, once per checkpoint, and is an INPUT of the kernel like the cosines.
    -> namespace(cos, clip_score, clip_ref, final, best, top2_margin, and the parts the bars need: scale, sp, v_ctl, rep)."""
    pr = np.asarray(probs, dtype=np.float64)
    B, K = pr.shape
    c = cosines(cos[0], cos[1], B) if isinstance(cos, tuple) else np.asarray(cos, dtype=np.float64)
    s = float(np.exp(np.float64(logit_scale))) if scale is None else float(scale)
    clip = softmax(c * s)
    al, be, ga = _col(alpha, B), _col(beta, B), _col(gamma, B)
    ctl = np.broadcast_to(np.asarray(control), (B,))
    final = al * pr + be * clip
    sp = np.zeros((B, K))
    v_ctl = np.zeros((B, K))
    rep = np.zeros((B, K))
    for b in range(B):
        if ctl[b] == 1:
            v_ctl[b] = np.asarray(senti_raw, dtype=np.float64)[b]
            rep[b] = 0.1 * (1.0 - np.exp(np.asarray(repeats, dtype=np.float64)[b]))
        elif ctl[b] == 2:
            v_ctl[b] = np.asarray(senti_raw, dtype=np.float64)[b] / 0.1
        if ctl[b]:
            sp[b] = softmax(v_ctl[b:b + 1])[0]
            final[b] = final[b] + ga[b] * sp[b] + rep[b]
    return SimpleNamespace(cos=c, clip_score=clip, clip_ref=c, final=final, best=np.argmax(final, axis=1),
                           top2_margin=top2_margin(final), scale=s, sp=sp, v_ctl=v_ctl, rep=rep, probs=pr, alpha=al, beta=be,
                           gamma=ga, control=ctl, repeats=None if repeats is None else np.asarray(repeats, dtype=np.float64))


def write_back(inp, cand, best, cols):
    """the rows after the step: inp[b, cols[b]] = cand[b, best[b]] (cols: one column, or [B])"""
    out = np.array(inp, copy=True)
    B = out.shape[0]
    cols = np.broadcast_to(np.asarray(cols), (B,))
    out[np.arange(B), cols] = np.asarray(cand)[np.arange(B), np.asarray(best)]
    return out


# ---- the bars (module docstring) --------------------------------------------------------------------------------------------------

def sum_roundings(K):
    return -(-int(K) // 256) + 14


def gamma_n(n):
    return n * U / (1.0 - n * U)


def softmax_bar(v, elem_err):
    """(a): v [B, K] the exact logits, elem_err [B, K] the bound on the error of each logit as the kernel holds it -> |error|
    allowed per element of softmax_K(v)"""
    v = np.asarray(v, dtype=np.float64)
    p = softmax(v)
    E = np.asarray(elem_err, dtype=np.float64) + U * np.abs(v - v.max(axis=1, keepdims=True))
    E = E + (p * E).sum(axis=1, keepdims=True)
    return np.expm1(E + gamma_n(sum_roundings(v.shape[1]))) * p + FLOOR


def clip_rel_bar(K, s, cabs=1.0):
    """(b): the worst relative error of clip_score over cosines |c| <= cabs, cosine-input mode"""
    return float(np.expm1(6.0 * U * s * cabs + gamma_n(sum_roundings(K))))


def final_bar_worst(K, s, alpha=0.02, beta=2.0, cabs=1.0):
    """(e) without control, at probs = clip = 1: absolute"""
    return abs(beta) * (clip_rel_bar(K, s, cabs) + FLOOR) + U * (abs(alpha) + abs(beta) + abs(alpha) + abs(beta))


def bars(r, feature_mode=False):
    """r: what combine() returned -> namespace(clip_score [B, K], clip_ref [B, K], final [B, K]) of allowed |error|"""
    s = r.scale
    e = U * s * np.abs(r.cos) + (s * COS_BAR if feature_mode else 0.0)
    b_clip = softmax_bar(r.cos * s, e)
    b_ref = np.full(r.cos.shape, COS_BAR) if feature_mode else REF_ULPS * np.spacing(np.abs(r.cos).astype(np.float32)).astype(np.float64)
    t1, t2 = r.alpha * r.probs, r.beta * r.clip_score
    b = np.abs(r.beta) * b_clip + U * (np.abs(t1) + np.abs(t2) + np.abs(t1 + t2))
    on = (r.control != 0)[:, None]
    pos = (r.control == 2)[:, None]
    sen = (r.control == 1)[:, None]
    b_sp = softmax_bar(r.v_ctl, np.where(pos, 3.0 * U * np.abs(r.v_ctl), 0.0))
    t3 = r.gamma * r.sp
    b = b + np.where(on, np.abs(r.gamma) * b_sp + U * (np.abs(t3) + np.abs(t1 + t2 + t3)), 0.0)
    if sen.any():
        er = np.exp(np.where(sen, r.repeats if r.repeats is not None else 0.0, 0.0))
        b = b + np.where(sen, 0.1 * (2 * U * er + U * np.abs(1.0 - er)) + 2 * U * np.abs(r.rep) + U * np.abs(r.final), 0.0)
    return SimpleNamespace(clip_score=b_clip, clip_ref=b_ref, final=b)


def sure_rows(r, b):
    """rows whose reference winner the kernel must reproduce: top-2 margin above twice the row's largest final bar"""
    return r.top2_margin > 2.0 * b.final.max(axis=1)


# ---- the inputs of tests/test_combine_kernel_gpu.py (tests/test_combine_ref_cpu.py asserts the winner shares on these arrays) -------

COS_KS = (1, 2, 63, 64, 255, 256, 257, 511, 1000, 1024)
COS_B = 4
FEAT_DS = (1, 63, 64, 65, 96, 512, 768)
FEAT_KS = (5, 257)
FEAT_B = 3
FEAT_WIDE = (257, 8, 64)   # B, K, D
CONTROL_HYPER = {0: (0.02, 2.0, 0.0), 1: (0.02, 2.0, 5.0), 2: (0.02, 2.0, 5.0)}   # alpha, beta, gamma per control mode
# every generator below draws from seed 0 unless a test passes its own: seed 0 meets the winner rule in every case
MIXED_KS = (200, 257)
MIXED_B = 9
ALPHAS, BETAS, GAMMAS = (0.0, 0.02, 1.0), (0.0, 1.0, 2.0), (0.0, 0.5, 5.0)


def fluency(rng, B, K):
    lg = rng.standard_normal((B, K)) * 2.0
    pr = np.exp(lg - lg.max(axis=1, keepdims=True))
    return (pr / pr.sum(axis=1, keepdims=True)).astype(np.float32)


def control_scores(rng, B, K, control):
    """sentiment: raw in +-20 and repeats as small integers of both signs; POS: raw in [0, 1]"""
    if control == 1:
        return (rng.uniform(-20.0, 20.0, (B, K)).astype(np.float32), rng.integers(-2, 4, (B, K)).astype(np.float32))
    if control == 2:
        return rng.uniform(0.0, 1.0, (B, K)).astype(np.float32), None
    return None, None


def cos_case(K, control, span=False, B=COS_B, seed=None):
    """cosines uniform in [-0.4, 0.4] (span: spanning exactly [-1, 1], K >= 2) -> dict(cos, probs, senti_raw, repeats, cand)"""
    rng = np.random.default_rng([0 if seed is None else seed, K, control, int(span)])
    if span:
        cos = rng.uniform(-1.0, 1.0, (B, K)).astype(np.float32)
        cos[:, K // 3] = -1.0
        cos[:, (2 * K) // 3 if K > 2 else 1] = 1.0
    else:
        cos = rng.uniform(-0.4, 0.4, (B, K)).astype(np.float32)
    sr, rp = control_scores(rng, B, K, control)
    return dict(cos=cos, probs=fluency(rng, B, K), senti_raw=sr, repeats=rp, cand=rng.integers(1, 30522, (B, K)).astype(np.int32))


def feat_case(K, D, B=FEAT_B, control=0, seed=None):
    """text features [B*K, D], image embeddings [B, D], standard normal"""
    rng = np.random.default_rng([0 if seed is None else seed, K, D, B])
    tf = rng.standard_normal((B * K, D)).astype(np.float32)
    ie = rng.standard_normal((B, D)).astype(np.float32)
    sr, rp = control_scores(rng, B, K, control)
    return dict(text_feat=tf, img=ie, probs=fluency(rng, B, K), senti_raw=sr, repeats=rp,
                cand=rng.integers(1, 30522, (B, K)).astype(np.int32))


def case_ref(case, logit_scale, control=0, feature_mode=False, scale=None):
    """the reference and its bars on a generated case under the control mode's hyper-parameters"""
    al, be, ga = (np.float64(np.float32(x)) for x in CONTROL_HYPER[control])
    cos = (case["text_feat"], case["img"]) if feature_mode else case["cos"]
    r = combine(cos, logit_scale, case["probs"], al, be, ga, control, case["senti_raw"], case["repeats"], scale=scale)
    return r, bars(r, feature_mode)


def mixed_case(B, K, seed=4):
    """B rows whose control is b % 3 (neighbours always differ) over every alpha, beta and gamma: a control-0 row carries a gamma the
    kernel must not use, and no row has alpha = beta = gamma = 0.  -> (hypers: [B] tuples (alpha, beta, gamma, control), case)"""
    hs = []
    for b in range(B):
        i, j = (b // 3) % 3, b % 3
        hs.append((ALPHAS[i], BETAS[(i + j + 1) % 3], GAMMAS[(i + 2 * j) % 3], j))
    rng = np.random.default_rng([seed, B, K])
    c1, c2 = control_scores(rng, B, K, 1), control_scores(rng, B, K, 2)
    ctl = np.arange(B) % 3
    sr = np.where((ctl == 2)[:, None], c2[0], c1[0]).astype(np.float32)
    case = dict(cos=rng.uniform(-0.4, 0.4, (B, K)).astype(np.float32), probs=fluency(rng, B, K), senti_raw=sr, repeats=c1[1],
                cand=rng.integers(1, 30522, (B, K)).astype(np.int32))
    return hs, case


def mixed_ref(hypers, case, logit_scale, scale=None):
    """the reference and its bars on a mixed_case under its per-row hyper-parameters (as the fp32 values a record holds)"""
    al, be, ga = (np.array([h[i] for h in hypers], np.float32).astype(np.float64) for i in range(3))
    ctl = np.array([h[3] for h in hypers], np.int64)
    r = combine(case["cos"], logit_scale, case["probs"], al, be, ga, ctl, case["senti_raw"], case["repeats"], scale=scale)
    return r, bars(r)


def left_out(r, b):
    """(share of rows left out of the winner comparison, rows kept)"""
    sure = sure_rows(r, b)
    return 1.0 - sure.mean(), int(sure.sum())


def planted_ties(K, at, B=3):
    """cosine-input rows whose scores tie exactly at the columns `at` (and nowhere else reach that value): probs are equal over the
    row and the cosines are 0.25 at `at`, below 0.2 elsewhere, so equal inputs give equal fp32 scores whatever the arithmetic"""
    rng = np.random.default_rng([7, K])
    cos = rng.uniform(-0.4, 0.2, (B, K)).astype(np.float32)
    cos[:, list(at)] = np.float32(0.25)
    probs = np.full((B, K), np.float32(1.0 / K), np.float32)
    return dict(cos=cos, probs=probs, senti_raw=None, repeats=None, cand=rng.integers(1, 30522, (B, K)).astype(np.int32))


def dominant_winner(K, k_star, B=3):
    """cosine-input rows on which column k_star wins by a margin far above any bar: cosine 0.4 against at most 0.1"""
    rng = np.random.default_rng([8, K])
    cos = rng.uniform(-0.4, 0.1, (B, K)).astype(np.float32)
    cos[:, k_star] = np.float32(0.4)
    return dict(cos=cos, probs=fluency(rng, B, K), senti_raw=None, repeats=None, cand=rng.integers(1, 30522, (B, K)).astype(np.int32))
