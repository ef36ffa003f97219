"""Every GEMM family on strided, windowed and in-place buffers (czc_test_gemm_layout), the launches the engine makes and the older
GEMM hooks never did: leading dimensions that differ from the widths and from one another, an output that is a column window of
wider rows (the last tower layer's k/v projection), a residual that IS the output (the fp32 residual stream), two outputs.

For each row of the table below -- the smallest shape at which the family has more than one tile or block in each direction and
a ragged edge in each -- the layouts run on the same numbers and, in this order of importance:
  1. the launcher reports the family the case was written for (kernel switches pinned with czc_test_set_option and restored);
  2. owned elements are BIT-EQUAL to the dense launch served by that family: a row's value does not depend on a leading dimension;
  3. the dense launch lies within the bound tests/test_kernels_gpu.py states for the family and precision (gemm_layout.bound);
  4. every pad column and guard row of every output still reads the 0x5a pattern, and no owned element is NaN;
  5. LayerNorm partials at part_ld > M equal those at part_ld == M, pad entries untouched.
tests/test_gemm_layout_cpu.py proves that the checker behind 2-5 (gemm_layout.check) can fail.  Each launch prints one line
`gemm-layout | row | layout | family` (pytest -s)."""
import functools
from dataclasses import replace

import numpy as np
import pytest

import gemm_layout as GL
import kernel_hooks as KH
from conzic_amd import native
from gemm_layout import BF16, F32, FP16, SPLIT, Case
from kernel_hooks import GEMM_OPTION_DEFAULTS as DEFAULTS, gemm_options as options  # noqa: F401

pytestmark = pytest.mark.gpu

HALF = [BF16, FP16]
NAME = {BF16: "bf16", F32: "f32", SPLIT: "split", FP16: "fp16"}


@functools.lru_cache(maxsize=None)
def _inputs(base):
    """dense fp32 inputs and the fp64 reference of a table row, computed once"""
    data = GL.make_data(base)
    ref = GL.reference(base, data)
    ref.setflags(write=False)
    return data, ref


def _report(row, name, launch):
    c = launch.case
    print(f"gemm-layout | {row} {NAME[c.prec]} {c.M}x{c.N}x{c.K} act={c.act} out={'+'.join(c.outputs())} | {name} "
          f"(lda {c.lda} ldw {c.ldw} ldc {c.ldc} ldr {c.ldr} c0 {c.c0}{' in place' if c.in_place else ''}) | {GL.FAMILY[launch.family]}")


def layouts_of(base):
    out = {"strided": base.strided(), "window": base.window()}
    if base.has_resid:
        out["in_place"] = base.inplace()
    return out


def x16_layouts(base):
    """the 2-byte residual stream runs in place, as the engine runs it; and once with a residual buffer of its own"""
    M, N = base.M, base.N
    return {"strided": replace(base.inplace(), part_ld=M + 5), "window": replace(base, c0=8, ldc=N + 24, in_place=True, part_ld=M + 5),
            "in_place": replace(base.inplace(), part_ld=M), "strided, own residual buffer": replace(base.strided(in_place=False), part_ld=M + 5)}


def run_row(row, base, family, opts, layouts=None, dense_family=None):
    data, ref = _inputs(replace(base, in_place=False, part_ld=0))
    with options(**opts):
        dense, _ = KH.gemm_layout(base, data)
        _report(row, "dense", dense)
        GL.check(dense, None, ref, expect_family=dense_family or family, data=data)
        for name, case in (layouts_of(base) if layouts is None else layouts).items():
            launch, _ = KH.gemm_layout(case, data)
            _report(row, name, launch)
            GL.check(launch, dense, ref, expect_family=family, data=data)
            if case.part_ld:
                GL.check_partials(launch, dense)
    return dense


# ---- the tiled kernel --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [F32, BF16, FP16, SPLIT])
@pytest.mark.parametrize("out", ["f32+resid", "typed", "both"])
def test_tiled_vec(prec, out):
    base = Case(prec, 130, 136, 64, resid=out != "typed", typed=out == "typed", both=out == "both", act=1 if out == "typed" else 0)
    run_row("tiled, vec", base, "tiled-vec", {})


@pytest.mark.parametrize("prec", [F32, BF16, FP16, SPLIT])
def test_tiled_scalar_by_n(prec):
    """N % 4 != 0 (the MLM decoder's form): dense is scalar too; ldc = 31 puts every row but each fourth off a 4-byte-pair boundary"""
    base = Case(prec, 67, 30, 64, resid=True)
    lay = {"strided": replace(base, lda=72, ldw=80, ldc=31, ldr=33).filled(), "window": replace(base, c0=1, ldc=35, ldr=37).filled(),
           "in_place": replace(base, lda=72, ldw=80, ldc=31, in_place=True).filled()}
    run_row("tiled, scalar by N % 4", base, "tiled-scalar", {}, lay)
    if prec != SPLIT:  # a split_t row is made of whole groups of 8
        typed = replace(base, resid=False, typed=True, act=1)
        run_row("tiled, scalar by N % 4", typed, "tiled-scalar", {},
                {"strided": replace(typed, lda=72, ldw=80, ldc=31).filled(), "window": replace(typed, c0=1, ldc=35).filled()})


@pytest.mark.parametrize("prec", [F32, BF16, FP16, SPLIT])
def test_tiled_scalar_by_ld(prec):
    """N % 4 == 0 but ldc or ldr is not: the dense launch of this shape is the VECTOR form, and the scalar form on odd leading
    dimensions must give its bits (same accumulators, same order of bias, activation and residual)"""
    base = Case(prec, 67, 32, 64, resid=True)
    lay = {"strided": replace(base, lda=72, ldw=80, ldc=34, ldr=38).filled(), "strided, only ldr odd": replace(base, ldc=56, ldr=38).filled(),
           "window": replace(base, c0=1, ldc=34, ldr=38).filled(), "in_place": replace(base, lda=72, ldw=80, ldc=34, in_place=True).filled()}
    run_row("tiled, scalar by ld % 4", base, "tiled-scalar", {}, lay, dense_family="tiled-vec")


@pytest.mark.parametrize("resid", [False, True])
def test_split_k(resid):
    run_row("split-K", Case(SPLIT, 130, 136, 2048, resid=resid), "split-K", {})


@pytest.mark.parametrize("M", [1, 17, 32])
@pytest.mark.parametrize("out", ["f32+resid", "typed"])
def test_skinny(M, out):
    base = Case(SPLIT, M, 40, 64, resid=out != "typed", typed=out == "typed", act=1 if out == "typed" else 0)
    lay = layouts_of(base)
    if out != "typed":  # ldc % 4 != 0: the kernel's scalar stores
        lay["strided, odd ldc"] = replace(base, lda=72, ldw=80, ldc=43, ldr=45).filled()
    run_row("skinny", base, "skinny", {}, lay)


# ---- the ring kernels --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", HALF)
@pytest.mark.parametrize("variant,family", [(3, "ring-loader"), (5, "ring-pingpong")])
@pytest.mark.parametrize("out", ["typed", "f32", "f32+resid", "both"])
def test_ring(prec, variant, family, out):
    base = Case(prec, 300, 264, 128, resid=out in ("f32+resid", "both"), typed=out == "typed", both=out == "both",
                act=0 if out == "f32+resid" else 1)
    run_row("ring", base, family, {"gemm256": variant, "gemm256_min_m": 1})


@pytest.mark.parametrize("out", ["typed", "f32+resid"])
def test_ring_split(out):
    base = Case(SPLIT, 300, 264, 64, resid=out != "typed", typed=out == "typed", act=1 if out == "typed" else 0)
    run_row("ring split", base, "ring-split", {"gemm256s_min_m": 1})


@pytest.mark.parametrize("prec", HALF)
def test_ring_x16(prec):
    base = Case(prec, 300, 512, 128, form=GL.X16, in_place=True, part_ld=300)
    run_row("ring x16", base, "ring-pingpong", {"gemm256_min_m": 1}, x16_layouts(base))


@pytest.mark.parametrize("prec", HALF)
def test_tiled_x16(prec):
    """the same layer below the ring kernel's row threshold: the tiled kernel's 2-byte epilogue"""
    base = Case(prec, 300, 512, 128, form=GL.X16, in_place=True, part_ld=300)
    run_row("tiled x16", base, "tiled-vec", {}, x16_layouts(base))


# ---- the weight-stationary kernels -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", HALF)
@pytest.mark.parametrize("act", [0, 1])
def test_wreg(prec, act):
    run_row("wreg", Case(prec, 70, 264, 512, typed=True, act=act), "wreg", {})


@pytest.mark.parametrize("prec", HALF)
def test_wreg_resid(prec):
    base = Case(prec, 70, 512, 512, form=GL.X16, in_place=True, part_ld=70)
    run_row("wreg-resid", base, "wreg-resid", {"wreg_resid_min_m": 1}, x16_layouts(base))


@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("in_kernel", [0, 1])
@pytest.mark.parametrize("act", [0, 1])
def test_wreg_lnf(prec, in_kernel, act):
    """the folded-LayerNorm consumer, statistics from ln_finalize_kernel and formed in the kernel (70 rows: three row blocks, one per
    work-group, so gemm_wreg_stats_in_kernel allows it)"""
    base = Case(prec, 70, 1024, 512, form=GL.LNF, act=act)
    run_row(f"wreg-lnf stats {'in kernel' if in_kernel else 'by ln_finalize'}", base, "wreg-lnf", {"wreg_stats_in_kernel": in_kernel})


@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("in_kernel", [0, 1])
def test_wreg_lnf_kv_window_of_the_last_tower_layer(prec, in_kernel):
    """The engine's own launch (csrc/engine.hip, the pooled last layer): k and v of the qkv projection alone -- N = 2H into rows 3H
    wide, the output H columns in, W and bias H rows in -- must give the k / v columns of the dense 3H-wide launch bit for bit and
    leave the q columns alone."""
    H = 512
    qkv = Case(prec, 70, 3 * H, H, form=GL.LNF)
    data, ref = _inputs(qkv)
    kv = replace(qkv, N=2 * H, c0=H, ldc=3 * H).filled()
    kv_data = dict(data, W=data["W"][H:], bias=data["bias"][H:])
    with options(wreg_stats_in_kernel=in_kernel):
        dense, _ = KH.gemm_layout(qkv, data)
        _report("wreg-lnf", "dense, 1536 wide", dense)
        GL.check(dense, None, ref, expect_family="wreg-lnf", data=data)
        launch, _ = KH.gemm_layout(kv, kv_data)
        _report("wreg-lnf", "k/v window", launch)
    GL.check(launch, None, ref[:, H:], expect_family="wreg-lnf", data=kv_data)
    es = 2
    assert np.array_equal(launch.owned_bytes("out_act"), dense.owned_bytes("out_act")[:, H * es:]), "k / v columns differ from the dense launch"


# ---- the full-row kernel -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", HALF)
@pytest.mark.parametrize("K", [64, 2048])
def test_rowln(prec, K):
    """ldc = 512 = N is required (so no window); the dense launch is in place as the engine runs it, the others vary lda, ldw and
    -- with a residual buffer of its own -- ldr"""
    base = Case(prec, 130, 512, K, form=GL.ROWLN, in_place=True)
    lay = {"strided": replace(base, lda=K + 8, ldw=K + 16, in_place=False, ldr=552).filled(),
           "in_place": replace(base, lda=K + 8, ldw=K + 16).filled(),
           "own residual buffer, dense": replace(base, in_place=False).filled()}
    run_row("rowln", base, "rowln", {"rowln_min_m": 1}, lay)


# ---- what eligibility refuses ------------------------------------------------------------------------------------------------------

def _refused(row, case, data, opts, not_family):
    with options(**opts):
        launch, family = KH.gemm_layout(case, data)
    _report(row + " REFUSED", "ineligible", launch)
    assert GL.FAMILY[family] not in not_family, GL.FAMILY[family]
    return launch, family


@pytest.mark.parametrize("prec", HALF)
def test_both_outputs_are_not_served_by_wreg(prec):
    base = Case(prec, 70, 264, 512, both=True, resid=False)
    dense = run_row("wreg, both outputs", base, "tiled-vec", {}, {"strided": base.strided(), "window": base.window()})
    assert GL.FAMILY[dense.family] != "wreg"


def test_both_outputs_are_not_served_by_ring_split():
    base = Case(SPLIT, 300, 264, 64, both=True, resid=True)
    dense = run_row("ring split, both outputs", base, "tiled-vec", {"gemm256s_min_m": 1})
    assert GL.FAMILY[dense.family] != "ring-split"


def test_leading_dimensions_that_a_family_refuses_fall_to_one_that_serves_them():
    """ld % 8 != 0 is outside the ring, weight-stationary and full-row kernels: the launcher must send the layout to the tiled kernel
    (and still be right there), or refuse it where only one family serves the form"""
    for row, base, opts, fam in (("ring", Case(BF16, 300, 264, 128, resid=True), {"gemm256": 5, "gemm256_min_m": 1}, "ring-pingpong"),
                                 ("ring split", Case(SPLIT, 300, 264, 64, resid=True), {"gemm256s_min_m": 1}, "ring-split"),
                                 ("wreg", Case(FP16, 70, 264, 512, typed=True), {}, "wreg")):
        data, ref = _inputs(base)
        with options(**opts):
            dense, _ = KH.gemm_layout(base, data)
        assert GL.FAMILY[dense.family] == fam
        case = replace(base, ldc=base.N + 4, ldr=base.N + 4 if base.resid else 0).filled()   # ldc % 8 == 4
        launch, family = _refused(row, case, data, opts, (fam,))
        assert GL.FAMILY[family] == "tiled-vec"
        GL.check(launch, None, ref, data=data)
    # one family only: the launcher refuses, nothing runs
    lnf = Case(FP16, 70, 1024, 512, form=GL.LNF)
    data, _ = _inputs(lnf)
    launch, family = _refused("wreg-lnf", replace(lnf, ldc=1028).filled(), data, {}, ("wreg-lnf",))
    assert family == 0 and launch.outside_untouched("out_act") == (True, True) and KH.untouched(launch.owned_bytes("out_act").copy().view(np.uint32)).all()
    rl = Case(BF16, 130, 512, 64, form=GL.ROWLN)
    data, _ = _inputs(rl)
    launch, family = _refused("rowln", replace(rl, ldc=536, ldr=552).filled(), data, {"rowln_min_m": 1}, ("rowln",))
    assert family == 0 and all(KH.untouched(np.ascontiguousarray(b).view(np.uint32)).all() for b in launch.values())
