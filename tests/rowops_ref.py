"""Host references of the row kernels (csrc/rowops.hip, csrc/ragged.hip): float64 numpy, or exact float32 / float16 numpy where a
result is bit-defined, and the forward-error bounds the GPU results are held to.  No GPU, no torch.

THE LAYERNORM BOUND.  u = 2^-24 is the unit roundoff of fp32 (one rounded operation: fl(a op b) = (a op b)(1 + d), |d| <= u).
The kernels form, for a row x of H values, all in fp32 and in SOME fixed tree order:

    mean = (sum x) / H;   d_i = x_i - mean;   var = (sum d_i^2) / H;   rstd = rsqrt(var + eps);   y_i = d_i * rstd * g_i + b_i

Write a = mean|x| = (sum |x_i|) / H and L = log2 H + 1.

 1. Mean.  A sum of H terms over a tree of depth log2 H carries a relative error of at most (log2 H) u against sum |x_i|, the
    division one more rounding:  dm = |mean^ - mean| <= L u a.
 2. Centred values.  d_i^ = fl(x_i - mean^):  |d_i^ - d_i| <= dm + u (|x_i| + a)   (|mean^| <= a(1 + L u)).
 3. Variance.  sum d_i^2 is a sum of non-negative terms: squares (one rounding each), the tree (log2 H), the division (one), so the
    arithmetic costs (L + 1) u RELATIVE to var.  The perturbation of the d_i: the common part -(mean^ - mean) is orthogonal to d
    (sum d_i = 0) and enters in second order only, as dm^2; the individual roundings u |d_i^| cost 2 u var.  Together
        dv = |var^ - var| <= (L + 3) u var + dm^2.
 4. rstd.  w = var + eps, one more rounding; rsqrt of the device is good to 1 ulp = 2 u relative.  d(w^-1/2) / w^-1/2 = dw / 2w:
        rho = |rstd^ - rstd| / rstd <= (dv + u w) / (2 w) + 2 u        (for var >> eps:  (L + 4) u / 2 + 2 u + dm^2 / 2 var).
 5. Output.  y_i^ = fl(fl(fl(d_i^ rstd^) g_i) + b_i): three roundings (fewer where the compiler fuses a multiply-add), of which the
    two products are relative to |d_i rstd g_i| and the last to |y_i|:
        |y_i^ - y_i| <= |g_i| rstd ( dm + u (|x_i| + a) + |d_i| (rho + 2 u) ) + u |y_i|.
    With |d_i| <= |x_i| + a this is the form  |gamma| rstd (|x| + mean|x|) c u  +  2 u |y|  (one u |y| is kept in hand for the
    products' cross terms); all second-order terms are covered by the factor SECOND = 1.01 (L u < 1e-6).

A constant row has d_i = 0 exactly when its mean is exact (H * value and the division are exact, e.g. 2.0): y = beta bit for bit.

A typed output rounds y^ once more to the storage type: half a unit in the last place at |y|: 2^-8 |y| for bf16 (8-bit significand:
spacing 2^-7 relative, half of it), 2^-11 |y| for fp16 (11 bits; floor 2^-25: the subnormal spacing is 2^-24), and for split hi + lo
(lo = fl16(y - hi) with |y - hi| <= 2^-11 |y|: half a spacing of lo is 2^-22 |y|, floor 2^-25) the looser 2^-21 |y|.  The rounding
acts on y^, so the term is taken at |y| + tol.

THE ln_finalize BOUND (statistics from 32-column partials, var = E[x^2] - mean^2 in fp32), against fp64 of the SAME partials:
S = sum of nblk partial sums, Q = sum of nblk partial sums of squares, each by nblk - 1 sequential adds: |S^ - S| <= (nblk - 1) u
sum |p_x|, |Q^ - Q| <= (nblk - 1) u Q.  mean^ = S^ / n: dm <= (nblk - 1) u (sum |p_x|) / n + u |mean|.  E2^ = Q^ / n: relative nblk u.
mean^2: relative 2 dm / |mean| + u.  The subtraction: one rounding of the difference.  So
    dv <= nblk u E2 + 2 |mean| dm + u mean^2 + u var,     E2 = var + mean^2:
relative to var this is ~ (nblk + 1) u (1 + mean^2 / var) + 2 (nblk) u mean^2 / var: the cancellation factor 1 + mean^2 / var.
rstd as in 4:  rho <= (dv + u w) / (2 w) + 2 u.  (The clamp of var^ at 0 only moves var^ towards var.)

THE l2_normalize BOUND.  s = sum x^2: per lane ceil(D / 64) sequential adds, 6 tree levels, one rounding per square: relative
(ceil(D / 64) + 7) u.  sqrt and the division are correctly rounded (u each):  |y^ - y| <= |y| ((ceil(D / 64) + 7) / 2 + 2) u.
"""
import numpy as np

U = 2.0 ** -24
SECOND = 1.01
BF16, F32, F16X3, F16 = 0, 1, 3, 4


# ---- storage types, exactly ---------------------------------------------------------------------------------------------------------
def bf16_bits(v):
    """float32 -> bf16 patterns, round to nearest even (finite values)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def f16_bits(v):
    return np.ascontiguousarray(v, np.float32).astype(np.float16).view(np.uint16)


def split_bits(v):
    """float32 -> (hi, lo) fp16 patterns: hi = fl16(v), lo = fl16(v - hi) (the subtraction is exact in fp32)"""
    v = np.ascontiguousarray(v, np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def store_bits(prec, v):
    """what a kernel that holds the float32 values v stores in precision `prec` (f32: the uint32 patterns)"""
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    if prec == F32:
        return v.view(np.uint32)
    return bf16_bits(v) if prec == BF16 else f16_bits(v) if prec == F16 else split_bits(v)


def bits_equal(a, b):
    if isinstance(a, tuple):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def storage_half_ulp(prec, y):
    """half a unit in the last place of the storage type at |y| (see the module comment)"""
    y = np.abs(y)
    if prec == F32:
        return np.zeros_like(y)
    if prec == BF16:
        return y * 2.0 ** -8
    if prec == F16:
        return np.maximum(y * 2.0 ** -11, 2.0 ** -25)
    return np.maximum(y * 2.0 ** -21, 2.0 ** -25)


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------
def row_stats64(x, eps):
    """x [M, H] -> mean, var, rstd in float64"""
    x = np.asarray(x, np.float64)
    m = x.mean(-1)
    v = ((x - m[:, None]) ** 2).mean(-1)
    return m, v, 1.0 / np.sqrt(v + eps)


def stats_bound(x, eps):
    """-> (mean, rstd, dm, rho): the fp64 statistics of the rows of x and the bounds on |mean^ - mean| and |rstd^ - rstd| / rstd of a
    two-pass fp32 computation in tree order (steps 1 - 4 of the module comment)"""
    x = np.asarray(x, np.float64)
    H = x.shape[-1]
    L = np.log2(H) + 1
    m, v, r = row_stats64(x, eps)
    a = np.abs(x).mean(-1)
    dm = L * U * a
    dv = (L + 3) * U * v + dm * dm
    w = v + eps
    rho = (dv + U * w) / (2 * w) + 2 * U
    return m, r, dm * SECOND, rho * SECOND


def layernorm64(x, gamma, beta, eps, row_idx=None):
    x = np.asarray(x, np.float64)
    if row_idx is not None:
        x = x[np.asarray(row_idx)]
    m, _, r = row_stats64(x, eps)
    return (x - m[:, None]) * r[:, None] * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def layernorm_bound(x, gamma, beta, eps, row_idx=None, prec=F32):
    """-> (y64, tol) [M, H]: the fp64 LayerNorm of the rows and the forward-error bound of an fp32 tree-order kernel on them, with
    the storage rounding of `prec` added (F32: none)"""
    x = np.asarray(x, np.float64)
    if row_idx is not None:
        x = x[np.asarray(row_idx)]
    g = np.asarray(gamma, np.float64)
    m, r, dm, rho = stats_bound(x, eps)
    a = np.abs(x).mean(-1)
    d = x - m[:, None]
    y = d * r[:, None] * g + np.asarray(beta, np.float64)
    tol = np.abs(g) * r[:, None] * (dm[:, None] + U * (np.abs(x) + a[:, None]) + np.abs(d) * (rho[:, None] + 2 * U)) + 2 * U * np.abs(y)
    tol = tol * SECOND
    return y, tol + storage_half_ulp(prec, np.abs(y) + tol)


def layernorm_f32(x, gamma, beta, eps, row_idx=None, mutant=None):
    """A float32 numpy LayerNorm in ANOTHER summation order than the kernels' (numpy's blocked pairwise sums over the whole row) -- the
    CPU stand-in of a correct kernel -- and its wrong variants (`mutant`): "no_eps", "h_minus_1", "one_pass", "gamma_shift",
    "no_row_idx"."""
    x = np.ascontiguousarray(x, np.float32)
    g, b = np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    if row_idx is not None and mutant != "no_row_idx":
        x = x[np.asarray(row_idx)]
    elif row_idx is not None:
        x = x[:len(row_idx)]
    H = np.float32(x.shape[1] - 1 if mutant == "h_minus_1" else x.shape[1])
    mean = x.sum(-1, dtype=np.float32) / H
    if mutant == "one_pass":
        var = np.maximum((x * x).sum(-1, dtype=np.float32) / H - mean * mean, np.float32(0))
    else:
        d = x - mean[:, None]
        var = (d * d).sum(-1, dtype=np.float32) / H
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = np.float32(1) / np.sqrt(var + (np.float32(0) if mutant == "no_eps" else np.float32(eps)), dtype=np.float32)
        if mutant == "gamma_shift":
            g, b = np.roll(g, 4), np.roll(b, 4)
        return ((x - mean[:, None]) * rstd[:, None] * g + b).astype(np.float32)


MUTANTS = ("no_eps", "h_minus_1", "one_pass", "gamma_shift", "no_row_idx")
LN_H = (4, 64, 320, 512, 768, 1024)
LN_M = (1, 4, 5, 37)
LN_EPS = (1e-5, 1e-12)
N_SRC = 50


def ln_inputs(H, seed=0):
    """50 source rows [N_SRC, H]: row 0 ordinary (3 N(0,1) + 0.5), row 1 mean 30 / spread 0.1, row 2 constant 2.0, then alternating
    ordinary / mean-30 rows; gamma, beta; and 37 picks with repeats out of the 50 (the first three pick rows 2, 1, 2)."""
    rng = np.random.default_rng(1000 * H + seed)
    x = (rng.standard_normal((N_SRC, H)) * 3 + 0.5).astype(np.float32)
    far = (30 + 0.1 * rng.standard_normal((N_SRC, H))).astype(np.float32)
    x[1::2] = far[1::2]
    x[2] = 2.0
    g = (1 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal(H)).astype(np.float32)
    idx = rng.integers(0, N_SRC, 37).astype(np.int32)
    idx[:3] = (2, 1, 2)
    idx[5] = idx[4]
    return x, g, b, idx


def inside(y, y64, tol):
    """per row: every value within its bound (a NaN is outside)"""
    return (np.abs(np.asarray(y, np.float64) - y64) <= tol).all(-1)


def worst_ratio(y, y64, tol):
    return float((np.abs(np.asarray(y, np.float64) - y64) / tol).max())


# ---- ln_finalize --------------------------------------------------------------------------------------------------------------------
LNF_RATIOS = (0.0, 1.0, 4.0, 16.0)


def lnf_inputs(M, ld, seed=0):
    """fp16 rows [M, 512] whose mean / spread ratio cycles through LNF_RATIOS (row i: LNF_RATIOS[i % 4]) -> (rows as float32, ratio
    per row, partials [16, ld, 2] float32: (sum, sum of squares) of the stored values per 32-column block, rounded once from fp64)"""
    rng = np.random.default_rng(77 + M + seed)
    ratio = np.array([LNF_RATIOS[i % 4] for i in range(M)])
    x = (ratio[:, None] + rng.standard_normal((M, 512))).astype(np.float16).astype(np.float64)
    blk = x.reshape(M, 16, 32)
    part = np.zeros((16, ld, 2), np.float32)
    part[:, :M, 0] = blk.sum(-1).T
    part[:, :M, 1] = (blk * blk).sum(-1).T
    return x.astype(np.float32), ratio, part


def ln_finalize_bound(part, M, eps):
    """part [nblk, ld, 2] float32 -> (mean, rstd, dm, rho) against fp64 of the same partials (module comment)"""
    p = np.asarray(part, np.float64)[:, :M]
    nblk = p.shape[0]
    n = nblk * 32.0
    S, Q = p[..., 0].sum(0), p[..., 1].sum(0)
    m, E2 = S / n, Q / n
    v = np.maximum(E2 - m * m, 0.0)
    w = v + eps
    dm = (nblk - 1) * U * np.abs(p[..., 0]).sum(0) / n + U * np.abs(m)
    dv = nblk * U * E2 + 2 * np.abs(m) * dm + U * m * m + U * v
    rho = (dv + U * w) / (2 * w) + 2 * U
    return m, 1.0 / np.sqrt(w), dm * SECOND, rho * SECOND


# ---- l2_normalize --------------------------------------------------------------------------------------------------------------------
def l2_normalize_bound(x):
    x = np.asarray(x, np.float64)
    D = x.shape[-1]
    y = x / np.sqrt((x * x).sum(-1, keepdims=True))
    return y, np.abs(y) * (((D + 63) // 64 + 7) / 2.0 + 2) * U * SECOND


# ---- embeddings, exactly --------------------------------------------------------------------------------------------------------------
def bert_embed_rows(ids, positions, word, pos, type0):
    """float32 (word[id] + type0) + pos[p] per (id, position): single IEEE adds, the kernels' order"""
    w = np.asarray(word, np.float32)[np.asarray(ids).reshape(-1)]
    return (w + np.asarray(type0, np.float32)) + np.asarray(pos, np.float32)[np.asarray(positions).reshape(-1)]


def clip_embed_rows(ids, seg_src, seg_pos0, own_off, own_len, tok, pos, n_out_rows):
    """-> (x [n_out_rows, H] float32 = tok[id] + pos[p] on the rows of the plan, written [n_out_rows] bool)"""
    tok, pos = np.asarray(tok, np.float32), np.asarray(pos, np.float32)
    x = np.zeros((n_out_rows, tok.shape[1]), np.float32)
    written = np.zeros(n_out_rows, bool)
    for s in range(len(own_len)):
        for i in range(int(own_len[s])):
            p = int(seg_pos0[s]) + i
            r = int(own_off[s]) + i
            x[r] = tok[int(ids[int(seg_src[s]), p])] + pos[p]
            written[r] = True
    return x, written


def im2col_ref(pix, p):
    """[B, 3, S, S] -> [B * (S/p)^2, 3*p*p]: patches[b*P + py*G + px][c*p*p + iy*p + ix] = pix[b][c][py*p + iy][px*p + ix]"""
    pix = np.asarray(pix, np.float32)
    B, C, S, _ = pix.shape
    G = S // p
    return pix.reshape(B, C, G, p, G, p).transpose(0, 2, 4, 1, 3, 5).reshape(B * G * G, C * p * p)


def vision_assemble_ref(patch_out, cls, pos):
    """[B, P, H], [H], [P + 1, H] -> [B, P + 1, H] float32: x[b, 0] = cls + pos[0], x[b, 1 + j] = patch_out[b, j] + pos[1 + j]"""
    po = np.asarray(patch_out, np.float32)
    B, P, H = po.shape
    e = np.concatenate([np.broadcast_to(np.asarray(cls, np.float32), (B, 1, H)), po], axis=1)
    return e + np.asarray(pos, np.float32)
