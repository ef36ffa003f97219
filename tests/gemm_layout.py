"""Host side of the GEMM layout tests (CPU only, numpy): the cases, the padded buffers, the fp64 reference and the checker.

A case is one GEMM launch whose leading dimensions, output window and aliasing are chosen by the test (czc_test_gemm_layout,
include/conzic_hip_test.h).  Every 2-D buffer of the hook -- and of the numpy emulation below, which lays its host arrays out the
same way -- has GUARD_ROWS rows in front of its rows, back_rows(rows) behind them and ld - width pad columns; operands hold NaNs
there, outputs the 0x5a pattern (kernel_hooks.SENTINEL), and outputs come back whole and raw.

  reference(case, data)    fp64 product of the operands AS ROUNDED TO THE OPERAND TYPE, with bias, activation and residual
  bound(case, name, ref)   the bound tests/test_kernels_gpu.py states for that family and precision (pointers at each line)
  check(launch, dense, ref)  owned elements against the dense launch (bit for bit) and the reference; pad columns and guard rows
                           still SENTINEL; no NaN in an owned element.  Raises LayoutError, whose .kind names what failed.
  emulate(case, data, fault)  a strided GEMM in numpy with index arithmetic on flat buffers, and the faults a kernel could have:
                           tests/test_gemm_layout_cpu.py proves with them that check() can fail.
"""
from dataclasses import dataclass, replace

import numpy as np

from kernel_hooks import SENTINEL, untouched

BF16, F32, SPLIT, FP16 = 0, 1, 3, 4                  # include/conzic_hip.h CZC_PREC_*
PLAIN, X16, LNF, ROWLN = 0, 1, 2, 3                  # CZC_GEMM_FORM_*
IN_PLACE, BOTH_OUTPUTS, TYPED_OUT = 1, 2, 4          # CZC_GEMM_* flags
GUARD_ROWS = 8                                       # CZC_TEST_LAYOUT_GUARD
FAMILY = {0: "none", 1: "tiled-vec", 2: "tiled-scalar", 3: "split-K", 4: "skinny", 5: "ring-loader", 6: "ring-pingpong",
          7: "ring-split", 8: "wreg", 9: "wreg-lnf", 10: "wreg-resid", 11: "rowln"}   # CZC_GEMM_FAMILY_*
FAMILY_ID = {v: k for k, v in FAMILY.items()}
ELEM_BYTES = {"f32": 4, "bf16": 2, "f16": 2, "split": 4}
KIND_OF_PREC = {BF16: "bf16", F32: "f32", SPLIT: "split", FP16: "f16"}


def back_rows(rows):
    """guard rows behind `rows` rows: to the end of the last 256-row tile, and GUARD_ROWS more"""
    return (-rows) % 256 + GUARD_ROWS


@dataclass(frozen=True)
class Case:
    prec: int
    M: int
    N: int
    K: int
    form: int = PLAIN
    act: int = 0
    resid: bool = False
    bias: bool = True
    typed: bool = False          # plain form: out_act only
    both: bool = False           # plain form: out_f32 and out_act
    in_place: bool = False
    lda: int = 0                 # 0: dense (K, K, c0 + N, c0 + N)
    ldw: int = 0
    ldc: int = 0
    ldr: int = 0
    c0: int = 0
    part_ld: int = 0             # x16: row_part with this leading dimension (0: none)

    def filled(self):
        """the same case with every leading dimension spelt out"""
        ldc = self.ldc or self.c0 + self.N
        return replace(self, lda=self.lda or self.K, ldw=self.ldw or self.K, ldc=ldc,
                       ldr=(ldc if self.in_place else (self.ldr or self.c0 + self.N)) if self.has_resid else 0)

    @property
    def has_resid(self):
        return self.resid or self.form in (X16, ROWLN)

    @property
    def flags(self):
        return (IN_PLACE if self.in_place else 0) | (BOTH_OUTPUTS if self.both else 0) | (TYPED_OUT if self.typed else 0)

    def outputs(self):
        """name -> element kind of every output buffer of the launch"""
        act_kind = KIND_OF_PREC[self.prec]
        if self.form == X16:
            return {"out_f32": "f16"}
        if self.form == LNF:
            return {"out_act": act_kind}
        if self.form == ROWLN or self.both:
            return {"out_f32": "f32", "out_act": act_kind}
        return {"out_act": act_kind} if self.typed else {"out_f32": "f32"}

    # the layouts of the issue, from the dense case of a table row
    def strided(self, **kw):
        return replace(self, lda=self.K + 8, ldw=self.K + 16, ldc=self.N + 24, ldr=self.N + 40 if self.has_resid else 0, **kw).filled()

    def window(self, c0=8):
        return replace(self, c0=c0, ldc=self.N + 24, ldr=self.N + 40 if self.has_resid else 0).filled()

    def inplace(self):
        return replace(self, lda=self.K + 8, ldw=self.K + 16, ldc=self.N + 24, ldr=self.N + 24, in_place=True).filled()


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & np.uint32(0xFFFF0000)).view(np.float32)


def f16_round(a):
    return np.ascontiguousarray(a, np.float32).astype(np.float16).astype(np.float32)


def operand_round(prec, a):
    """an fp32 array as the device holds it in the operand type (split-fp16 keeps ~22 bits: fp32-class, left as it is, the
    convention of tests/test_kernels_gpu.py::test_split_fp16_gemm_is_fp32_class)"""
    return bf16_round(a) if prec == BF16 else f16_round(a) if prec == FP16 else np.ascontiguousarray(a, np.float32)


def make_data(case, seed=0):
    """dense fp32 inputs of a case; a function of (precision, form, M, N, K) and the seed only, so that every layout of a table
    row runs on the same numbers"""
    c = case
    rng = np.random.default_rng([seed, c.prec, c.form, c.M, c.N, c.K])
    d = {"A": rng.standard_normal((c.M, c.K)).astype(np.float32),
         "W": (rng.standard_normal((c.N, c.K)) * 0.05).astype(np.float32),
         "bias": rng.standard_normal(c.N).astype(np.float32),
         "resid": (rng.standard_normal((c.M, c.N)) * 1.5).astype(np.float32)}
    if c.form == LNF:
        d["A"] = (d["A"] * 2).astype(np.float32)
        d["A"][::7] += 6.0          # |mean| = 3 sigma (tests/test_kernels_gpu.py::test_layernorm_folded_into_the_weight_stationary_gemm)
        d["gamma"] = (1 + 0.2 * rng.standard_normal(c.K)).astype(np.float32)
        d["beta"] = (0.1 * rng.standard_normal(c.K)).astype(np.float32)
        blk = f16_round(d["A"]).astype(np.float64).reshape(c.M, c.K // 32, 32)
        d["ln_part"] = np.ascontiguousarray(np.stack([blk.sum(-1), (blk * blk).sum(-1)], axis=-1).transpose(1, 0, 2), np.float32)
    if c.form == ROWLN:
        d["gamma"] = (1.0 + 0.3 * rng.standard_normal(c.N)).astype(np.float32)
        d["beta"] = (0.2 * rng.standard_normal(c.N)).astype(np.float32)
    return d


def activation(x, act):
    if act == 1:
        return x / (1.0 + np.exp(-1.702 * x))
    assert act == 0
    return x


def reference(case, data):
    """fp64 value of every owned output element BEFORE its rounding to the output type -> [M, N].  (rowln: x; its LayerNorm
    output is referred to the launch's own x, see rowln_y_reference.)"""
    c = case
    b = data["bias"].astype(np.float64) if c.bias else 0.0
    if c.form == LNF:
        x = f16_round(data["A"]).astype(np.float64)
        mu = x.mean(1, keepdims=True)
        y = (x - mu) / np.sqrt(x.var(1, keepdims=True) + 1e-5) * data["gamma"] + data["beta"]
        return activation(y @ data["W"].astype(np.float64).T + b, c.act)
    acc = operand_round(c.prec, data["A"]).astype(np.float64) @ operand_round(c.prec, data["W"]).astype(np.float64).T + b
    if c.form == X16:
        return acc + f16_round(data["resid"]).astype(np.float64)
    return activation(acc, c.act) + (data["resid"].astype(np.float64) if c.has_resid else 0.0)


def rowln_y_reference(x, data, eps=1e-5):
    x64 = x.astype(np.float64)
    mu = x64.mean(1, keepdims=True)
    return (x64 - mu) / np.sqrt(x64.var(1, keepdims=True) + eps) * data["gamma"] + data["beta"]


def bound(case, name, ref):
    """|output - ref| allowed per owned element, as tests/test_kernels_gpu.py states it for the family and precision"""
    c, k = case, np.sqrt(case.K / 64)
    typed = name == "out_act"
    a = np.abs(ref)
    if c.form == X16:     # test_residual_gemm_on_fp16_rows: one fp16 rounding of the result + fp32 summation order
        return np.maximum(a, 1.0) * 2.0 ** -10 + 2e-4 * k
    if c.form == LNF:     # test_layernorm_folded_into_the_weight_stationary_gemm
        return np.maximum(a, 1.0) * (2.0 ** -8 if c.prec == BF16 else 2.0 ** -10) + 6e-3
    if c.form == ROWLN:   # test_full_row_gemm_with_layernorm_epilogue (mean_shift 0): x, and y against the LayerNorm of x
        if typed:
            return (2.0 ** -8 if c.prec == BF16 else 2.0 ** -11) * a + 2e-5
        return np.full_like(a, 2e-4 * np.sqrt(max(c.K, 512) / 512))
    if c.prec == BF16:    # test_gemm_asymmetric; test_gemm_weight_stationary: + one bf16 rounding of a typed output
        return 2e-3 * k + (a * 2.0 ** -8 if typed else 0.0)
    if c.prec == FP16:    # test_fp16_gemm_kernel_families
        return np.full_like(a, 3e-4 * k + (2.0 ** -10 * a.max() if typed else 0.0))
    if c.prec == F32:     # test_gemm_asymmetric
        return np.full_like(a, 2e-5 * k)
    return np.full_like(a, 4e-5 * k)  # split: test_split_fp16_gemm_is_fp32_class, 1e-5 sqrt(K / 64) * 4


# ---- buffers --------------------------------------------------------------------------------------------------------------------

class Launch(dict):
    """name -> the WHOLE raw buffer of an output, uint8 [GUARD_ROWS + M + back_rows(M), ldc * element bytes]; .case (filled),
    .family (CZC_GEMM_FAMILY_*, 0: the launcher refused), .part / .part_guards (x16 with part_ld: [N / 32, part_ld, 2] and the
    hook's guard words)"""

    def __init__(self, case, family=0):
        super().__init__()
        self.case, self.family, self.part, self.part_guards = case.filled(), family, None, None

    def total_rows(self):
        return GUARD_ROWS + self.case.M + back_rows(self.case.M)

    def owned_bytes(self, name):
        c, es = self.case, ELEM_BYTES[self.case.outputs()[name]]
        return self[name][GUARD_ROWS:GUARD_ROWS + c.M, c.c0 * es:(c.c0 + c.N) * es]

    def owned(self, name):
        """owned elements as fp64 [M, N]"""
        kind = self.case.outputs()[name]
        raw = np.ascontiguousarray(self.owned_bytes(name))
        if kind == "f32":
            v = raw.view(np.float32)
        elif kind == "f16":
            v = raw.view(np.float16)
        elif kind == "bf16":
            v = (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
        else:  # split_t: groups of 8 elements = 16 bytes of fp16 hi parts, then 16 bytes of lo parts
            h = raw.view(np.float16).astype(np.float64).reshape(self.case.M, -1, 2, 8)
            return (h[:, :, 0, :] + h[:, :, 1, :]).reshape(self.case.M, self.case.N)
        return v.astype(np.float64)

    def outside_untouched(self, name):
        """(pads ok, guards ok): every byte of the buffer outside the owned elements still holds the pre-fill pattern -- pad
        columns of the M rows / guard rows"""
        c, es = self.case, ELEM_BYTES[self.case.outputs()[name]]
        buf = self[name]
        rows = buf[GUARD_ROWS:GUARD_ROWS + c.M]
        pads = np.concatenate([rows[:, :c.c0 * es], rows[:, (c.c0 + c.N) * es:]], axis=1).reshape(-1)
        guards = np.concatenate([buf[:GUARD_ROWS].reshape(-1), buf[GUARD_ROWS + c.M:].reshape(-1)])
        return _all_untouched(pads), _all_untouched(guards)


def _all_untouched(b):
    b = np.ascontiguousarray(b, np.uint8)
    n4 = b.size // 4 * 4
    return bool(untouched(b[:n4].view(np.uint32)).all()) and bool((b[n4:] == (SENTINEL & 0xFF)).all())


def padded(dense, ld, c0, fill, dtype=np.float32):
    """the rows of `dense` inside a host buffer laid out as the hook lays its device buffers out -> flat array, and the index of
    element (0, 0)"""
    rows, width = dense.shape
    buf = np.full((GUARD_ROWS + rows + back_rows(rows), ld), fill, dtype)
    buf[GUARD_ROWS:GUARD_ROWS + rows, c0:c0 + width] = dense
    return buf.reshape(-1), GUARD_ROWS * ld + c0


class LayoutError(AssertionError):
    def __init__(self, kind, msg):
        super().__init__(f"[{kind}] {msg}")
        self.kind = kind


def check(launch, dense, ref, expect_family=None, data=None, bit_equal=True):
    """The assertions of a layout launch, most important first.  dense: the Launch of the same table row on dense buffers served
    by the same family (None: this IS the dense launch).  ref: reference(case, data).  Raises LayoutError(kind):
      family   the launcher chose another family than the test was written for
      dense    an owned element differs from the dense launch (bit for bit; bit_equal=False skips it for a pair the test holds to
               the fp64 bound only)
      ref      an owned element is outside bound() of the fp64 reference
      pad / guard   a pad column / guard row of an output no longer reads SENTINEL
      nan      an owned element is NaN"""
    c = launch.case
    if expect_family is not None and launch.family != FAMILY_ID[expect_family]:
        raise LayoutError("family", f"{c}: served by {FAMILY.get(launch.family, launch.family)}, not {expect_family}")
    for name in c.outputs():
        if dense is not None and bit_equal and not np.array_equal(launch.owned_bytes(name), dense.owned_bytes(name)):
            d = np.argwhere(launch.owned(name) != dense.owned(name))
            raise LayoutError("dense", f"{c} {name}: {len(d)} owned elements differ from the dense launch, first (row, col) {d[:4].tolist()}")
    for name in c.outputs():
        out = launch.owned(name)
        if np.isnan(out).any():
            raise LayoutError("nan", f"{c} {name}: NaN in owned elements {np.argwhere(np.isnan(out))[:4].tolist()}")
        r = rowln_y_reference(launch.owned("out_f32"), data) if (c.form == ROWLN and name == "out_act") else ref
        bad = np.abs(out - r) > bound(c, name, r)
        if bad.any():
            raise LayoutError("ref", f"{c} {name}: {int(bad.sum())} owned elements outside the bound, worst {float(np.abs(out - r).max()):.3e}, "
                                     f"first (row, col) {np.argwhere(bad)[:4].tolist()}")
    for name in c.outputs():
        pads_ok, guards_ok = launch.outside_untouched(name)
        if not pads_ok:
            raise LayoutError("pad", f"{c} {name}: a store landed in a pad column")
        if not guards_ok:
            raise LayoutError("guard", f"{c} {name}: a store landed in a guard row")


def check_partials(launch, dense):
    """row_part at part_ld > M: the rows equal those at part_ld == M, the pad entries and the guard words are untouched"""
    c = launch.case
    if not np.array_equal(launch.part[:, :c.M], dense.part[:, :dense.case.M]):
        raise LayoutError("dense", f"{c}: LayerNorm partials differ from the launch with part_ld == M")
    if not (untouched(launch.part[:, c.M:]).all() and untouched(launch.part_guards).all()):
        raise LayoutError("pad", f"{c}: a partial landed in a pad entry or a guard word")
    if not np.isfinite(launch.part[:, :c.M]).all() or untouched(launch.part[:, :c.M]).any():
        raise LayoutError("nan", f"{c}: a partial of an owned row was not written")


# ---- a strided GEMM in numpy, and what a kernel could get wrong ---------------------------------------------------------------------

FAULTS = ("ldr_as_ldc", "K_as_lda", "pad_store", "row_M_store", "nan_pad_read", "in_place_overlap")
# fault -> the LayoutError.kind that check() names it by (against the dense launch, on its own)
EXPECTED_KIND = {"ldr_as_ldc": ("dense", "ref"), "K_as_lda": ("dense", "nan"), "pad_store": ("pad", "pad"), "row_M_store": ("guard", "guard"),
                 "nan_pad_read": ("dense", "nan"), "in_place_overlap": ("dense", "ref")}


def emulate(case, data, fault=None, tile_n=16):
    """f32 plain-form launch (fp32 output) by index arithmetic `row * ld + col` on flat host buffers laid out like the hook's, one
    tile_n-column tile after the other.  Faults:
      ldr_as_ldc        the store uses the residual's leading dimension
      K_as_lda          the A rows are taken K apart
      pad_store         one store into column N of a row (a pad column / the next column of a wider row)
      row_M_store       one store into row M
      nan_pad_read      one A element is fetched from its row's first pad column
      in_place_overlap  the ragged last tile is moved back to overlap its neighbour, as a kernel that only handles whole tiles
                        would: harmless out of place, but in place it adds the residual that its neighbour has ALREADY stored"""
    assert fault is None or fault in FAULTS
    c = case.filled()
    assert c.prec == F32 and c.form == PLAIN and not c.typed and not c.both
    m, k = np.arange(c.M), np.arange(c.K)
    A, a0 = padded(data["A"], c.lda, 0, np.nan)
    W, w0 = padded(data["W"], c.ldw, 0, np.nan)
    F = np.full((GUARD_ROWS + c.M + back_rows(c.M)) * c.ldc, SENTINEL, np.uint32).view(np.float32)
    f0 = GUARD_ROWS * c.ldc + c.c0
    R, r0, ldr = None, 0, c.ldr
    if c.has_resid and c.in_place:
        F.reshape(-1, c.ldc)[GUARD_ROWS:GUARD_ROWS + c.M, c.c0:c.c0 + c.N] = data["resid"]
        R, r0 = F, f0
    elif c.has_resid:
        R, r0 = padded(data["resid"], c.ldr, c.c0, np.nan)
    lda = c.K if fault == "K_as_lda" else c.lda
    ldc = c.ldr if fault == "ldr_as_ldc" else c.ldc
    ia = a0 + m[:, None] * lda + k[None, :]
    if fault == "nan_pad_read":
        ia[min(3, c.M - 1), c.K - 1] += 1
    a = A[ia].astype(np.float64)
    for n0 in range(0, c.N, tile_n):
        if fault == "in_place_overlap" and n0 + tile_n > c.N:
            n0 = max(c.N - tile_n, 0)
        cols = np.arange(n0, min(n0 + tile_n, c.N))
        w = W[w0 + cols[:, None] * c.ldw + k[None, :]].astype(np.float64)
        v = activation(a @ w.T + (data["bias"][cols] if c.bias else 0.0), c.act)
        if R is not None:
            v = v + R[r0 + m[:, None] * ldr + cols[None, :]]
        F[f0 + m[:, None] * ldc + cols[None, :]] = v.astype(np.float32)
    if fault == "pad_store":
        F[f0 + min(5, c.M - 1) * c.ldc + c.N] = 1.0
    if fault == "row_M_store":
        F[f0 + c.M * c.ldc + 2] = 1.0
    out = Launch(c, FAMILY_ID["tiled-vec"])
    out["out_f32"] = F.view(np.uint8).reshape(-1, c.ldc * 4)
    return out
