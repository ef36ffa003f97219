"""Host side of the GEMM range tests (CPU only, numpy): operand constructions away from unit scale, the fp64 reference, a
scale-aware error unit, and a numpy model of a GEMM launch with the faults a kernel could have.

The older GEMM tests draw A ~ N(0, 1..2), W ~ 0.05 N(0, 1) and hold |out - ref| to an ABSOLUTE bound tuned to that scale
(gemm_layout.bound).  Such a bound sees one scale: at activation scale 3e-4 a kernel that returned zeros would pass it.  Here the
error of an element is counted in units of what fp32 accumulation of ITS OWN terms may cost.

THE UNIT.  ref is the fp64 result on the operands as the kernel reads them (bf16 / fp16 operands rounded to the type as
gemm_layout.operand_round does, fp32 and split operands the fp32 values), bias, activation and residual in fp64, and
    S = sum_k |a_k| |w_k| + |bias| + |resid|.
A kernel that forms exact products (11 x 11 or 8 x 8 significand bits fit fp32; the fp32 MFMA fuses) and adds them to an fp32
accumulator in ANY order errs by at most gamma_n * S, n the length of its longest chain (Higham, Accuracy and Stability, 4.2):
every addition rounds a partial sum whose magnitude is at most S by a relative 2^-24.  So with u = 2^-24
    e = max(0, |out - ref| - r_out(ref)) / (u * S + floor)
is at most n + 3 (bias add, residual add, and one more for the second-order terms of gamma_n while n u << 1) for ANY summation
order: the a-priori cap K_chain + 4 that every E below must respect.  r_out is what the ONE rounding to the output type may
add: half the spacing of the type at ref (bf16: 8 significand bits, fp16: 11, fp16 subnormal spacing 2^-24), 0 for fp32 output.
A split output is hi = fp16(v), lo = fp16(v - hi): r_out = half the fp16 spacing at (half the fp16 spacing at ref).

SPLIT OPERANDS.  v is held as hi + lo, two fp16 (csrc/common.h Act<split_t>): |v - (hi + lo)| <= 2^-22 |v| while lo is a normal
fp16 (2^-11 of 2^-11), and the kernels run three passes hi*hi + hi*lo + lo*hi, dropping lo*lo (<= 2^-22 |a||w|).  Per term:
2^-22 (a) + 2^-22 (w) + 2^-22 (lo*lo) = 3 * 2^-22 |a||w|, so u * S becomes (2^-24 + 3 * 2^-22) * S.  Where lo falls below the
smallest normal fp16 it is a multiple of 2^-24 and v - (hi + lo) is up to 2^-25 ABSOLUTE per operand element: the product sum moves
by at most floor = 2^-25 * sum_k (|a_k| + |w_k|)  (|da| |w| + |a| |dw| <= 2^-25 (|w| + |a|) while |a|, |w| <= 1; for larger operands
lo is normal and the relative term covers it).  The documented profile of the representation -- relative error 4e-7 at unit scale,
2e-6 at 0.01, 6e-5 at 3e-4 -- is this floor against |C| ~ sa sw sqrt(K), no longer three numbers.  The hardware must NOT flush
those subnormal lo parts: one_sided_lo(small=True) has them all of one sign, and flushing is then worth a whole cross pass.

THE FOLDED-LAYERNORM FORM (wreg-lnf) computes act(rstd_m * (x . W"^T) + b') on weights folded and centred by fold_ln_kernel.
The constructions give it gamma = 1, beta = 0 and fp16-exact weight rows that sum to zero exactly (antisymmetric halves), so the
fold is the identity and "the operands as the kernel reads them" are x (fp16), W and the fp32 partials ln_part; rstd is formed
in fp64 from those partials, and S = rstd * sum |x||w| + |bias|.

THE ACTIVATION SWEEP is not measured in units (its products are exact: one-hot rows): see act_bound().

The bound E per (family, precision) is 4 x the maximum of e measured on the MI355X over the whole matrix of
tests/test_gemm_range_gpu.py and seeds 0..2, rounded up (kernels are deterministic; the factor covers the tail of other seeds),
and must satisfy E <= K_chain + 4 and 2 E < every fault that claims() lists: tests/test_gemm_range_cpu.py asserts both.
"""
import functools
import math
import zlib

import numpy as np

from conzic_amd.harness import OUTLIER_CHANNELS
from gemm_layout import BF16, F32, FP16, LNF, ROWLN, SPLIT, X16, Case, bf16_round, f16_round, operand_round

U = 2.0 ** -24
U_SPLIT = 2.0 ** -24 + 3 * 2.0 ** -22
F16_MAX = 65504.0
F16_OVERFLOW = 65520.0      # the smallest magnitude that rounds to infinity
EDGE_MARGIN = 4.0           # x16_edge: distance kept from 65520 / 65504; > E u S = 516 * 2^-24 * 7e4 = 2.2 for every E allowed
LN_EPS = 1e-5

# ---- measured on the MI355X: max e over the matrix and seeds 0..2, and E = ceil(4 x max) ------------------------------------------
# (family, precision) -> (measured maximum, E).  The maxima of the half-precision and fp32 families come from the outlier and
# cancelling constructions (18.2 and 12.7 units at most; every scale pair stays below 5.4), those of the split families from
# the scale pairs and the one-sided constructions (all below 0.8); the x16 edge measures 0.79 at most.
E_TABLE = {
    ("tiled-vec", F32): (18.21, 73),
    ("tiled-scalar", F32): (17.69, 71),
    ("tiled-vec", BF16): (7.06, 29),
    ("tiled-scalar", BF16): (5.92, 24),
    ("tiled-vec", FP16): (7.19, 29),
    ("tiled-scalar", FP16): (5.73, 23),
    ("tiled-vec", SPLIT): (0.61, 3),
    ("tiled-scalar", SPLIT): (0.67, 3),
    ("split-K", SPLIT): (0.66, 3),
    ("skinny", SPLIT): (0.50, 2),
    ("ring-loader", BF16): (6.72, 27),
    ("ring-pingpong", BF16): (6.72, 27),
    ("wreg", BF16): (1.86, 8),
    ("wreg-resid", BF16): (3.40, 14),
    ("wreg-lnf", BF16): (0.43, 2),
    ("rowln", BF16): (7.57, 31),
    ("ring-loader", FP16): (6.49, 26),
    ("ring-pingpong", FP16): (6.49, 26),
    ("wreg", FP16): (2.84, 12),
    ("wreg-resid", FP16): (4.37, 18),
    ("wreg-lnf", FP16): (0.53, 3),
    ("rowln", FP16): (7.73, 31),
    ("ring-split", SPLIT): (0.77, 4),
}


def E(family, prec):
    return E_TABLE[(family, prec)][1]


def row_bound(family, c):
    """what a row of the matrix is held to: E of its family and precision, and never more than ITS OWN a-priori cap"""
    return min(E(family, c.prec), k_chain(c.prec, c.K) + 4)


def k_chain(prec, K):
    """the longest chain of fp32 additions one output element can have: K products, three passes for split operands"""
    return 3 * K if prec == SPLIT else K


# ---- number formats ---------------------------------------------------------------------------------------------------------------

def half_spacing(kind, x):
    """half the spacing of the output type at |x| (round to nearest may move a value by this much)"""
    a = np.abs(np.asarray(x, np.float64))
    if kind == "f32":
        return np.zeros_like(a)
    if kind == "split":
        return half_spacing("f16", half_spacing("f16", a))
    p, emin = {"bf16": (8, -126), "f16": (11, -14)}[kind]
    e = np.frexp(np.maximum(a, 2.0 ** emin))[1] - 1          # floor(log2 |x|), the smallest normal binade below it
    return np.ldexp(1.0, e - p)


def bf16_chop(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def f16_chop(a):
    a = np.ascontiguousarray(a, np.float32)
    r = a.astype(np.float16)
    over = np.abs(r.astype(np.float32)) > np.abs(a)
    r = np.where(over, np.nextafter(r, np.float16(0)), r)
    return r.astype(np.float32)


def split_planes(a, flush=False):
    """hi, lo fp16 planes of an fp32 array as Act<split_t>::st forms them (fp32 values)"""
    a = np.ascontiguousarray(a, np.float32)
    hi = f16_round(a)
    lo = f16_round(a - hi)
    if flush:
        lo = np.where(np.abs(lo) < 2.0 ** -14, np.float32(0), lo)
    return hi, lo


def round_out(kind, v, chop=False):
    v = np.ascontiguousarray(v, np.float32)
    if kind == "f32":
        return v.astype(np.float64)
    if kind == "bf16":
        return (bf16_chop(v) if chop else bf16_round(v)).astype(np.float64)
    if kind == "f16":
        return (f16_chop(v) if chop else f16_round(v)).astype(np.float64)
    hi = f16_chop(v) if chop else f16_round(v)
    return hi.astype(np.float64) + f16_round(v - hi).astype(np.float64)


def act64(x, act):
    x = np.asarray(x, np.float64)
    if act == 0:
        return x
    with np.errstate(over="ignore"):
        if act == 1:
            return x / (1.0 + np.exp(-1.702 * x))
    assert act == 2   # 0.5 x (1 + erf(x / sqrt 2)) = 0.5 x erfc(-x / sqrt 2): no cancellation in the negative tail
    return 0.5 * x * np.vectorize(math.erfc, otypes=[np.float64])(-x / math.sqrt(2.0))


# ---- constructions: each a function of (precision, form, M, N, K, seed) only ---------------------------------------------------------

SCALES = ((2.0, 0.05), (0.01, 1.0), (1.0, 5e-4), (0.01, 0.01), (3e-4, 1.0), (300.0, 0.05), (1.0, 30.0))


def _rng(name, c, seed):
    return np.random.default_rng([seed, zlib.crc32(name.encode()), c.prec, c.form, c.M, c.N, c.K])


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _finish(c, d, rng):
    if c.form == ROWLN:
        d["gamma"] = _f32(1.0 + 0.3 * rng.standard_normal(c.N))
        d["beta"] = _f32(0.2 * rng.standard_normal(c.N))
    if c.form == LNF:
        # gamma = 1, beta = 0, fp16-exact weight rows whose halves are mirror images: the row sums to zero exactly, the fold is the
        # identity (see the module docstring)
        h = c.K // 2
        W = f16_round(d["W"])
        W[:, h:] = -W[:, rng.permutation(h)]
        d["W"] = W
        d["gamma"], d["beta"] = np.ones(c.K, np.float32), np.zeros(c.K, np.float32)
        blk = f16_round(d["A"]).astype(np.float64).reshape(c.M, c.K // 32, 32)
        d["ln_part"] = _f32(np.stack([blk.sum(-1), (blk * blk).sum(-1)], axis=-1).transpose(1, 0, 2))
    return d


def scales(c, seed, sa, sw):
    """normal operands at activation scale sa and weight scale sw; bias and residual at the scale of the product"""
    rng = _rng(f"scales {sa} {sw}", c, seed)
    mag = sa * sw * math.sqrt(c.K)
    d = {"A": _f32(rng.standard_normal((c.M, c.K)) * sa), "W": _f32(rng.standard_normal((c.N, c.K)) * sw),
         "bias": _f32(rng.standard_normal(c.N) * mag), "resid": _f32(rng.standard_normal((c.M, c.N)) * 1.5 * mag)}
    return _finish(c, d, rng)


def _unit(c, rng):
    return {"A": _f32(rng.standard_normal((c.M, c.K))), "W": _f32(rng.standard_normal((c.N, c.K)) * 0.05),
            "bias": _f32(rng.standard_normal(c.N)), "resid": _f32(rng.standard_normal((c.M, c.N)) * 1.5)}


def outliers(c, seed, side):
    """the outlier channels of a trained checkpoint (harness.outlier_clip_weights): those columns of A (side 'a') or W ('w') x 100"""
    rng = _rng("outliers " + side, c, seed)
    d = _unit(c, rng)
    ch = np.unique(np.array(OUTLIER_CHANNELS) % c.K)
    d["A" if side == "a" else "W"][:, ch] *= np.float32(100)
    return _finish(c, d, rng)


def cancelling(c, seed):
    """four pairs of terms +T, -T, T = 1024 x the rest, the partners K / 2 apart: S is large and |ref| small, and whatever rounds a
    partial sum to 16 bits between the partners (a split-K slab, a ring hand-over) shows.  x 32 on both operands is exact in every
    operand type, the partner columns are copies (A) and negations (W): the pairs cancel exactly."""
    rng = _rng("cancelling", c, seed)
    d = _unit(c, rng)
    h = c.K // 2
    k = rng.choice(h, size=4, replace=False)
    d["A"][:, k] *= np.float32(32)
    d["W"][:, k] *= np.float32(32)
    d["A"][:, k + h] = d["A"][:, k]
    d["W"][:, k + h] = -d["W"][:, k]
    return _finish(c, d, rng)


def one_sided_lo(c, seed, side, small=False):
    """split precision: one operand = h (1 + 2^-13), h > 0 fp16-exact, so every lo part is positive; the other operand positive and
    fp16-exact, so every lo part is zero.  A missing cross pass errs with one sign everywhere.  small: h in [2^-4, 2^-3), so every lo
    part is a SUBNORMAL fp16 (128..256 quanta of 2^-24): hardware that flushed them would lose the whole pass."""
    assert c.prec == SPLIT
    rng = _rng(f"one_sided_lo {side} {small}", c, seed)
    shape_l, shape_o = ((c.M, c.K), (c.N, c.K)) if side == "a" else ((c.N, c.K), (c.M, c.K))
    h = f16_round(rng.uniform(2.0 ** -4, 2.0 ** -3, shape_l) if small else rng.uniform(1.0, 2.0, shape_l))
    v = _f32(h * np.float32(1 + 2.0 ** -13))
    other = f16_round(rng.uniform(0.5, 1.5, shape_o) if small else rng.uniform(0.05, 0.15, shape_o))
    hi, lo = split_planes(v)
    assert np.array_equal(v.astype(np.float64), h.astype(np.float64) * (1 + 2.0 ** -13)), "h (1 + 2^-13) is not exact in fp32"
    assert np.array_equal(hi, h) and (lo > 0).all() and (not small or (lo < 2.0 ** -14).all())
    oh, ol = split_planes(other)
    assert np.array_equal(oh, other) and (ol == 0).all() and (other > 0).all()
    d = {"A": v if side == "a" else other, "W": other if side == "a" else v,
         "bias": np.zeros(c.N, np.float32), "resid": np.zeros((c.M, c.N), np.float32)}
    return _finish(c, d, rng)


ACT_GRID = np.concatenate([0.5 * np.arange(256), -0.5 * np.arange(256)])   # exact in every operand type


def act_sweep(c, seed, with_bias):
    """Row m of A is one-hot at k = m mod ceil(512 / N) (k = 0 for N >= 512) and W[n, k] walks the grid +-0.5 j, j = 0..255, so the
    pre-activations of every ceil(512 / N) consecutive rows are the whole grid -127.5 .. 127.5, each formed from ONE exact product;
    the other entries of the used W columns hold the same grid, the unused columns noise (times an exact zero).  with_bias adds a
    small fp32 bias, so that the pre-activations leave the grid and the bias add rounds.
    The folded-LayerNorm form normalises A, so there the grid sits in the BIAS: W = 0 (its rows sum to zero, the fold is the
    identity), A is noise, and the epilogue rstd * 0 + b hands the activation exactly b[n] = grid[n mod 512] (with_bias: the grid
    plus the small noise, as one fp32 value: nothing rounds in front of the activation in either variant)."""
    rng = _rng(f"act_sweep {with_bias}", c, seed)
    if c.form == LNF:
        grid = ACT_GRID[np.arange(c.N) % 512] + (rng.standard_normal(c.N) * 1e-3 if with_bias else 0.0)
        d = {"A": _f32(rng.standard_normal((c.M, c.K))), "W": np.zeros((c.N, c.K), np.float32), "bias": _f32(grid)}
        assert c.N >= 512
        return _finish(c, d, rng)
    slots = -(-512 // c.N)
    assert slots <= c.K and c.M >= slots
    A = np.zeros((c.M, c.K), np.float32)
    A[np.arange(c.M), np.arange(c.M) % slots] = 1
    W = _f32(rng.standard_normal((c.N, c.K)) * 0.05)
    for s in range(slots):
        W[:, s] = ACT_GRID[(np.arange(c.N) + s * c.N) % 512]
    d = {"A": A, "W": W, "bias": _f32(rng.standard_normal(c.N) * 1e-3) if with_bias else np.zeros(c.N, np.float32),
         "resid": np.zeros((c.M, c.N), np.float32)}
    return _finish(c, d, rng)


def x16_edge(c, seed):
    """The 2-byte residual stream at the top of fp16, four blocks of rows.
    [0, r1): resid in the binades 2^13 .. 2^15 (spacing 8 .. 32), A.W^T + b of order 1 to 10: the fp64 sum rounded ONCE, in units.
    [r1, r2): the fp64 sum lies in [65520 + margin, 70000], sign by row: +-inf (a saturating conversion would hide the overflow
      the engine reports as CZC_ERR_OVERFLOW).  Column 0 of W is 1 and A[m, 0] = +-256 there, so that every element clears 65520.
    [r2, r3): sums just below 65504 - margin: finite.
    [r3, M): ties.  The row of A is +-(e_1 + e_2) - e_3, W[n, 1] = 4 + 8 i, W[n, 2] = +-2^-9, W[n, 3] = bias[n] (a multiple of 1/16),
      resid = +-(2^13 + 8 j) with the sum below 2^14 (spacing 8): every partial sum in any order, the bias add and the residual add are EXACT in fp32, the sum is
      2^-9 off a tie of the fp16 grid, and the output must EQUAL the fp64 sum rounded once -- a kernel that rounds the product sum
      to fp16 first lands on the tie and goes the other way for half of them."""
    assert c.form == X16 and c.M >= 64 and c.K >= 4
    rng = _rng("x16_edge", c, seed)
    r1, r2, r3 = c.M - 56, c.M - 32, c.M - 16
    A = _f32(rng.standard_normal((c.M, c.K)))
    W = _f32(rng.standard_normal((c.N, c.K)) * (6.0 / math.sqrt(c.K)))
    bias = _f32(np.round(rng.standard_normal(c.N) * 16).clip(-63, 63) / 16)
    W[:, 0] = 1
    W[:, 1] = 4 + 8 * rng.integers(0, 3, c.N)
    W[:, 2] = rng.choice([-1.0, 1.0], c.N) * 2.0 ** -9
    W[:, 3] = bias
    sign = np.where(np.arange(c.M) % 2 == 0, 1.0, -1.0)[:, None]
    A[r1:r2, 0] = 256 * sign[r1:r2, 0]
    A[r3:] = 0
    A[r3:, 1:3] = sign[r3:]
    A[r3:, 3] = -1
    resid = rng.uniform(2.0 ** 13, 2.0 ** 15, (c.M, c.N)) * rng.choice([-1.0, 1.0], (c.M, c.N))
    resid[r1:r2] = rng.uniform(65408, F16_MAX, (r2 - r1, c.N)) * sign[r1:r2]
    resid[r2:r3] = rng.uniform(65024, 65408, (r3 - r2, c.N)) * rng.choice([-1.0, 1.0], (r3 - r2, c.N))
    resid[r3:] = (2.0 ** 13 + 8 * rng.integers(0, 1016, (c.M - r3, c.N))) * sign[r3:]
    d = {"A": A, "W": W, "bias": bias, "resid": f16_round(resid), "rows": (r1, r2, r3)}
    ref = reference(c, d)[0]
    assert np.isfinite(d["resid"]).all() and np.array_equal(d["resid"][r3:], resid[r3:])
    # what the tie rows multiply is exact in the operand type
    assert np.array_equal(operand_round(c.prec, A[r3:]), A[r3:]) and np.array_equal(operand_round(c.prec, W[:, :4]), W[:, :4])
    assert (np.abs(ref[r1:r2]) >= F16_OVERFLOW + EDGE_MARGIN).all() and (np.abs(ref[r1:r2]) <= 70000).all()
    assert (np.sign(ref[r1:r2]) == sign[r1:r2]).all()
    assert (np.abs(ref[r2:r3]) <= F16_MAX - EDGE_MARGIN).all() and (np.abs(ref[r2:r3]) >= 64900).all()
    assert (np.abs(ref[:r1]) <= 2.0 ** 15 + 100).all()
    assert (np.abs(ref[r3:]) < 2.0 ** 14).all(), "tie rows: the sum leaves the binade of spacing 8"
    assert (np.abs(np.abs(np.abs(ref[r3:]) % 8 - 4) - 2.0 ** -9) == 0).all(), "tie rows: the sum is not 2^-9 off a tie"
    return _finish(c, d, rng)


def constructions(c):
    """name -> constructor(case, seed) of every construction that applies to a case (act_sweep: see sweeps())"""
    out = {f"scales {sa:g} x {sw:g}": functools.partial(scales, sa=sa, sw=sw) for sa, sw in SCALES}
    if c.form == LNF:
        return out          # A is normalised by the kernel: the other constructions are statements about A
    out["outliers in A"] = functools.partial(outliers, side="a")
    out["outliers in W"] = functools.partial(outliers, side="w")
    out["cancelling"] = cancelling
    if c.prec == SPLIT:
        for side in "aw":
            out[f"one-sided lo in {side.upper()}"] = functools.partial(one_sided_lo, side=side)
            out[f"one-sided subnormal lo in {side.upper()}"] = functools.partial(one_sided_lo, side=side, small=True)
    if c.form == X16:
        out["x16 edge"] = x16_edge
    return out


# ---- the matrix of tests/test_gemm_range_gpu.py (here so that the CPU test runs the model at the same shapes) ----------------------

HALF = (BF16, FP16)
NAME = {BF16: "bf16", F32: "f32", SPLIT: "split", FP16: "fp16"}


def _matrix():
    """(row name, family, dense case, czc_test_set_option switches, K is fixed by the family): the dense row of each family in the
    table of tests/test_gemm_layout_gpu.py, at K of 64 / 256 / 512 where K is free"""
    rows = []
    for prec in (F32, BF16, FP16, SPLIT):
        f32r, typed = dict(resid=True), dict(typed=True)
        for K, out, var, opts in ((64, f32r, "64-wide deep", {}), (256, typed, "64-wide deep", {}), (512, f32r, "64-wide deep", {}),
                                  (256, f32r, "128-wide", {"gemm_deep": 0}), (256, typed, "128-wide deep", {"gemm_small_tiles": 0})):
            rows.append((f"tiled {var}", "tiled-vec", Case(prec, 133, 136, K, **out), opts, False))
        for K in (64, 256, 512):
            rows.append(("tiled scalar", "tiled-scalar", Case(prec, 67, 30, K, resid=True), {}, False))
    rows.append(("split-K", "split-K", Case(SPLIT, 133, 136, 2048, resid=True), {}, True))
    for M, K, out in ((16, 64, dict(resid=True)), (16, 1536, dict(resid=True)), (17, 64, dict(resid=True)), (17, 256, dict(typed=True))):
        rows.append((f"skinny M={M} K={K}", "skinny", Case(SPLIT, M, 40, K, **out), {}, K == 1536))
    for prec in HALF:
        for variant, family in ((3, "ring-loader"), (5, "ring-pingpong")):
            for K, out in ((64, dict(typed=True)), (64, dict(resid=True)), (128, dict(typed=True)), (256, dict(resid=True)), (512, dict(typed=True))):
                rows.append((family.replace("-", " "), family, Case(prec, 293, 264, K, **out), {"gemm256": variant, "gemm256_min_m": 1, "wreg": 0}, False))
        rows.append(("ring x16", "ring-pingpong", Case(prec, 300, 512, 128, form=X16, in_place=True, part_ld=300), {"gemm256_min_m": 1}, False))
        rows.append(("tiled x16", "tiled-vec", Case(prec, 300, 512, 128, form=X16, in_place=True, part_ld=300), {}, False))
        rows.append(("wreg", "wreg", Case(prec, 70, 264, 512, typed=True), {}, True))
        rows.append(("wreg-resid", "wreg-resid", Case(prec, 70, 512, 512, form=X16, in_place=True, part_ld=70), {"wreg_resid_min_m": 1}, True))
        rows.append(("wreg-lnf", "wreg-lnf", Case(prec, 70, 1024, 512, form=LNF), {}, True))
        for K in (64, 256, 512):
            rows.append(("rowln", "rowln", Case(prec, 133, 512, K, form=ROWLN, in_place=True), {"rowln_min_m": 1}, False))
    for K, out in ((64, dict(resid=True)), (256, dict(typed=True)), (512, dict(resid=True))):
        rows.append(("ring split", "ring-split", Case(SPLIT, 293, 264, K, **out), {"gemm256s_min_m": 1}, False))
    return rows


MATRIX = _matrix()
IDS = [f"{row}-{NAME[c.prec]}-{c.M}x{c.N}x{c.K}-{'+'.join(c.outputs())}".replace(" ", "_") for row, _, c, _, _ in MATRIX]


def applicable(c, fixed_k):
    return [n for n in constructions(c) if not n.startswith("one-sided") or c.K <= 256 or fixed_k]


# ---- reference and the unit -------------------------------------------------------------------------------------------------------

def reference(c, d):
    """(ref, S, floor) per owned element, fp64: see the module docstring"""
    b = d["bias"].astype(np.float64) if c.bias else np.zeros(c.N)
    floor = 0.0
    if c.form == LNF:
        x, W = f16_round(d["A"]).astype(np.float64), d["W"].astype(np.float64)
        part = d["ln_part"].astype(np.float64)
        mean = part[:, :, 0].sum(0) / c.K
        rstd = 1.0 / np.sqrt(np.maximum(part[:, :, 1].sum(0) / c.K - mean * mean, 0.0) + LN_EPS)
        return act64(rstd[:, None] * (x @ W.T) + b, c.act), rstd[:, None] * (np.abs(x) @ np.abs(W).T) + np.abs(b), floor
    A, W = operand_round(c.prec, d["A"]).astype(np.float64), operand_round(c.prec, d["W"]).astype(np.float64)
    pre, S = A @ W.T + b, np.abs(A) @ np.abs(W).T + np.abs(b)
    if c.prec == SPLIT:
        floor = 2.0 ** -25 * (np.abs(A).sum(1)[:, None] + np.abs(W).sum(1)[None, :])
    if c.has_resid:
        r = (f16_round(d["resid"]) if c.form == X16 else d["resid"]).astype(np.float64)
        return act64(pre, c.act) + r, S + np.abs(r), floor
    return act64(pre, c.act), S, floor


def units(c, kind, out, ref3):
    """e per element (module docstring); kind: the element type of the output"""
    ref, S, floor = ref3
    assert c.act == 0, "the unit is a statement about sums: activations are held by act_bound()"
    with np.errstate(invalid="ignore"):
        excess = np.maximum(0.0, np.abs(out - ref) - half_spacing(kind, ref))
    return excess / ((U_SPLIT if c.prec == SPLIT else U) * S + floor)


def check_x16_edge(c, d, out, ref3):
    """the overflow rows are infinite with the sign of the sum, every other row is finite, the tie rows EQUAL the fp64 sum rounded
    once -> e of the other finite rows"""
    r1, r2, r3 = d["rows"]
    ref = ref3[0]
    assert np.isinf(out[r1:r2]).all(), f"{c}: {int(np.isfinite(out[r1:r2]).sum())} sums beyond 65520 + {EDGE_MARGIN} came back finite (saturated?)"
    assert (np.sign(out[r1:r2]) == np.sign(ref[r1:r2])).all(), f"{c}: an overflow has the wrong sign"
    fin = np.ones(c.M, bool)
    fin[r1:r2] = False
    assert np.isfinite(out[fin]).all(), f"{c}: a sum below 65504 - {EDGE_MARGIN} came back non-finite"
    once = ref[r3:].astype(np.float16).astype(np.float64)       # numpy rounds fp64 -> fp16 once
    assert np.array_equal(out[r3:], once), f"{c}: {int((out[r3:] != once).sum())} exact sums next to a tie were not rounded once"
    return units(c, "f16", out[fin], (ref[fin], ref3[1][fin], 0.0))


# ---- the activation sweep ---------------------------------------------------------------------------------------------------------

# the activations each launcher instantiates (1 quick-GELU, 2 GELU by erf); split-K, the x16 forms and rowln take none
ACTS = {"tiled-vec": (1, 2), "tiled-scalar": (1, 2), "skinny": (1, 2), "ring-loader": (1,), "ring-pingpong": (1,), "ring-split": (1,),
        "wreg": (1,), "wreg-lnf": (1,), "split-K": (), "wreg-resid": (), "rowln": ()}


def act_bound(c, kind, d):
    """|out - ref| allowed per element of an act_sweep launch, from the forms in the code (v = the fp32 pre-activation).
    quick-GELU, half-precision families (csrc/gemm.hip apply_act, gemm256.hip act_fn, gemm_wreg.hip wr_act):
        v * rcp(1 + exp2(c2 * v)), c2 = fp32(-1.702 log2 e);   the others:  v / (1 + expf(c1 * v)), c1 = fp32(-1.702).
      The argument t = c * v carries the rounding of the constant and of the product (2 x 2^-24 relative; 3 with a bias, whose add
      rounds v itself), and the exponential turns a relative error of t into |t| ln 2 = 1.702 |v| times as much in its value:
      the dominating term at the ends.  sigma = 1 / (1 + E) moves by at most the relative error of E.  Then one ulp (2^-23) each
      for the exponential, the add, the reciprocal / division and the product with v: 4 ulps.  Where 1 + E overflows or sigma falls
      below the smallest normal fp32 the hardware returns 0: an absolute 2^-126 |v|.
    GELU (erf):  0.5 v (1 + erff(v / sqrt 2)).  1 + erf is formed with an ABSOLUTE error: erff 4 ulp of a value below 1 (4 x 2^-24),
      its argument's rounding (<= 3 x 2^-24 relative) times |z| erf'(z) <= 0.49, the add's 2^-24: 7 x 2^-24, times 0.5 |v|; and
      two ulps relative for the products.
    Every form: + the one rounding to the output type, and with a bias the rounding of v = w + b through the slope of the
    activation (|f'| <= 1.13): 2^-24 |v| * 1.13."""
    ref, _, _ = reference(c, d)
    v = np.abs(operand_round(c.prec, d["A"]).astype(np.float64) @ operand_round(c.prec, d["W"]).astype(np.float64).T + d["bias"].astype(np.float64))
    with_bias = bool(np.any(d["bias"])) and c.form != LNF     # lnf: the bias IS the pre-activation (act_sweep), no add rounds
    a = np.abs(ref)
    if c.act == 1:
        b = a * ((3 if with_bias else 2) * U * 1.702 * v + 4 * 2.0 ** -23) + 2.0 ** -126 * v
    else:
        b = 0.5 * v * 7 * U + a * 2 * 2.0 ** -23
    if with_bias:
        b = b + 1.13 * U * v
    return b + half_spacing(kind, ref)


# ---- a GEMM launch in numpy: the honest model and the faults ------------------------------------------------------------------------

FAULTS = ("trunc_operand", "trunc_out", "drop_lo_a", "drop_lo_w", "drop_lo_group", "flush_lo", "half_partial", "double_round", "saturate",
          "act_clamp")


def emulate(c, d, fault=None, block=None):
    """name -> output [rows, cols] (fp64 values of the output type) of the launch as an honest kernel would compute it: exact
    products added to ONE fp32 accumulator in ascending k (split: three passes lo_a*hi_w, hi_a*lo_w, hi*hi into the same
    accumulator), bias, activation, residual in fp32, one rounding to the output type.  block = (row indices, column indices)
    restricts it to those elements (they do not depend on one another).  Faults:
      trunc_operand   the operands are chopped to bf16 / fp16 instead of rounded to nearest
      trunc_out       the 16-bit (or split) output is chopped
      drop_lo_a / drop_lo_w   split: the pass with A's / W's lo parts is missing
      drop_lo_group   split: both cross passes skip the 32-wide k group in the middle of K
      flush_lo        split: subnormal lo parts read as zero
      half_partial    the partial sum at K / 2 is rounded to the operand type (bf16; fp16 for fp16 and split)
      double_round    x16: the product sum + bias is rounded to fp16 BEFORE the residual is added
      saturate        x16: the sum is clamped to +-65504 before the conversion
      act_clamp       the activation returns NaN beyond |v| = 88 (an exponential that overflows into inf / inf)"""
    assert fault is None or fault in FAULTS
    rows, cols = (np.arange(c.M), np.arange(c.N)) if block is None else block
    A, W = _f32(d["A"])[rows], _f32(d["W"])[cols]
    a_prec = FP16 if c.form == LNF else c.prec
    rnd = {BF16: bf16_chop, FP16: f16_chop}.get(a_prec) if fault == "trunc_operand" else None
    if c.prec == SPLIT:
        (ah, al), (wh, wl) = split_planes(A, fault == "flush_lo"), split_planes(W, fault == "flush_lo")
        if fault == "drop_lo_group":
            g = (c.K // 32) // 2
            al, wl = al.copy(), wl.copy()
            al[:, 32 * g:32 * g + 32] = 0
            wl[:, 32 * g:32 * g + 32] = 0
        passes = ([] if fault == "drop_lo_a" else [(al, wh)]) + ([] if fault == "drop_lo_w" else [(ah, wl)]) + [(ah, wh)]
    else:
        Ar = rnd(A) if rnd else operand_round(a_prec, A)
        Wr = rnd(W) if rnd and c.form != LNF else operand_round(FP16 if c.form == LNF else c.prec, W)
        passes = [(Ar, Wr)]
    part_round = {BF16: bf16_round, FP16: f16_round, SPLIT: f16_round}.get(c.prec) if fault == "half_partial" else None
    acc = np.zeros((len(rows), len(cols)), np.float32)
    for pa, pw in passes:
        pa, pw = pa.astype(np.float64), pw.astype(np.float64)
        for k in range(c.K):
            if part_round and k == c.K // 2:
                acc = part_round(acc)
            acc = (acc.astype(np.float64) + pa[:, k, None] * pw[None, :, k]).astype(np.float32)
    bias = (_f32(d["bias"])[cols] if c.bias else np.zeros(len(cols), np.float32)).astype(np.float64)
    if c.form == LNF:
        part = d["ln_part"].astype(np.float64)[:, rows]
        mean = part[:, :, 0].sum(0) / c.K
        rstd = (1.0 / np.sqrt(np.maximum(part[:, :, 1].sum(0) / c.K - mean * mean, 0.0) + LN_EPS)).astype(np.float32)
        acc = (rstd[:, None].astype(np.float64) * acc).astype(np.float32)
    v = (acc.astype(np.float64) + bias).astype(np.float32)
    if c.act:
        with np.errstate(invalid="ignore"):
            v = np.where((np.abs(v) > 88) & (fault == "act_clamp"), np.float32(np.nan), act64(v, c.act).astype(np.float32))
    kinds = c.outputs()
    if c.form == X16:
        r = f16_round(d["resid"])[np.ix_(rows, cols)].astype(np.float64)
        if fault == "double_round":
            v = f16_round(v)
        v = (v.astype(np.float64) + r).astype(np.float32)
        if fault == "saturate":
            v = np.clip(v, -F16_MAX, F16_MAX)
        with np.errstate(over="ignore"):
            return {"out_f32": round_out("f16", v, fault == "trunc_out")}
    if c.has_resid:
        v = (v.astype(np.float64) + _f32(d["resid"])[np.ix_(rows, cols)]).astype(np.float32)
    return {name: round_out(kind, v, fault == "trunc_out" and kind != "f32") for name, kind in kinds.items() if not (c.form == ROWLN and name == "out_act")}


# ---- which fault each construction separates ----------------------------------------------------------------------------------------
# construction (prefix of its name) -> the faults that tests/test_gemm_range_cpu.py proves to lie outside 2 E on at least one
# element, for the cases that meet the condition beside it.  What is NOT claimed, and why:
#   flush_lo on `scales`: with lo parts of random sign the flushed parts add like sqrt(K) while the floor of the unit (their
#     worst case) adds like K -- below one unit; only the one-sided subnormal construction separates it.
#   drop_lo_group beyond K = 256 and on split-K (K >= 2048): one 32-wide group of K is worth 2^-13 * 32 / K of S, 64 units of
#     2^-24 S at K = 512 against a chain of 16: claimed up to K = 256 only, so one_sided_lo runs at K <= 256 wherever K is free.
#   trunc_operand on split / fp32: there is no 16-bit operand rounding to get wrong.
def claims(c, cname):
    half, typed16 = c.prec in (BF16, FP16), any(k in ("bf16", "f16") for k in c.outputs().values())
    out = []
    if cname.startswith(("scales 2 x", "outliers")):
        out += ["trunc_operand"] if half or c.form == LNF else []
        out += ["trunc_out"] if typed16 and c.form != ROWLN and cname.startswith("scales") else []
    if cname == "cancelling" and c.prec != F32:
        out += ["half_partial"]
    if cname.startswith("one-sided"):
        side = cname[-1].lower()
        out += ["drop_lo_" + side] + (["drop_lo_group"] if c.K <= 256 else [])
        if "subnormal" in cname:
            out += ["flush_lo"]
    if cname == "x16 edge":
        out += ["saturate", "trunc_out", "double_round"]
    return out
