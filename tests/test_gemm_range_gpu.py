"""Every GEMM family against fp64 across operand scales and ranges (tests/gemm_range.py): the matrix is every family x every
precision it serves x every construction that applies, at the smallest shapes that still cross a tile edge (two ragged tiles of
M, a ragged tile of N where the family allows one, K of 64 / 256 / 512 or the family's fixed K).  Each launch goes through kernel_hooks.gemm_layout, which reports the family that
served it: every case asserts it.  An element's error is counted in units of its own fp32 accumulation error (gemm_range.units)
and held to gemm_range.row_bound = min(E(family, precision), the row's own K_chain + 4); the activation sweep to gemm_range.act_bound; the fp16 residual stream at the top
of its range to one rounding and an honest overflow.  tests/test_gemm_range_cpu.py proves that these checks can fail.
Each launch prints one line `gemm-range | row | construction | family | max e` (pytest -s)."""
import functools
from dataclasses import replace

import numpy as np
import pytest

import gemm_layout as GL
import gemm_range as GR
import kernel_hooks as KH
from gemm_range import NAME
from kernel_hooks import gemm_options as options

pytestmark = pytest.mark.gpu


MATRIX, IDS, applicable = GR.MATRIX, GR.IDS, GR.applicable


def _dense(c):
    return replace(c, in_place=False, part_ld=0)


@functools.lru_cache(maxsize=None)
def _range_inputs(key, cname, seed):
    """the operands of a construction and their fp64 reference, computed once and left unchanged"""
    data = GR.act_sweep(key, seed, cname.endswith("True")) if cname.startswith("act_sweep") else GR.constructions(key)[cname](key, seed)
    ref3 = GR.reference(key, data)
    for a in ref3:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return data, ref3


def measure(i, seed=0):
    """construction -> max e of matrix row i (every launch's family, overflow rows and rowln's LayerNorm output asserted)"""
    row, family, c, opts, fixed_k = MATRIX[i]
    out = {}
    with options(**opts):
        for cname in applicable(c, fixed_k):
            data, ref3 = _range_inputs(_dense(c), cname, seed)
            launch, fam = KH.gemm_layout(c, data)
            assert GL.FAMILY[fam] == family, f"{row} {c}: served by {GL.FAMILY.get(fam, fam)}, not {family}"
            name = "out_act" if "out_f32" not in launch else "out_f32"
            kind, got = c.outputs()[name], launch.owned(name)
            if cname == "x16 edge":
                e = GR.check_x16_edge(c, data, got, ref3)
            else:
                assert np.isfinite(got).all(), f"{row} {c} {cname}: non-finite output"
                e = GR.units(c, kind, got, ref3)
            if c.form == GL.ROWLN:   # the LayerNorm output keeps its check against the launch's own x
                y, yref = launch.owned("out_act"), GL.rowln_y_reference(got, data)
                assert (np.abs(y - yref) <= GL.bound(c, "out_act", yref)).all(), f"{row} {c} {cname}: LayerNorm output"
            out[cname] = float(e.max())
            print(f"gemm-range | {row} {NAME[c.prec]} {c.M}x{c.N}x{c.K} {name} | {cname} | {GL.FAMILY[fam]} | {out[cname]:.2f}")
    return out


@pytest.mark.parametrize("i", range(len(MATRIX)), ids=IDS)
def test_units(i):
    _, family, c, _, _ = MATRIX[i]
    worst, bound = measure(i), GR.row_bound(family, c)
    bad = {n: e for n, e in worst.items() if e > bound}
    assert not bad, f"{IDS[i]}: beyond {bound} units: {bad}"


SWEEPS = [(i, act) for i, (_, family, c, _, _) in enumerate(MATRIX) if c.form in (GL.PLAIN, GL.LNF) for act in GR.ACTS[family]]


def sweep(i, act, with_bias, seed=0):
    """max of |out - ref| / act_bound over an act_sweep launch of matrix row i"""
    row, family, base, opts, _ = MATRIX[i]
    c = replace(base, act=act, resid=False)
    data, _ = _range_inputs(c, f"act_sweep {with_bias}", seed)
    with options(**opts):
        launch, fam = KH.gemm_layout(c, data)
    assert GL.FAMILY[fam] == family, f"{row} {c}: served by {GL.FAMILY.get(fam, fam)}, not {family}"
    (name, kind), = c.outputs().items()
    got = launch.owned(name)
    assert np.isfinite(got).all(), f"{row} {c}: NaN or infinity at pre-activations {np.unique(GR.reference(replace(c, act=0), data)[0][~np.isfinite(got)])[:8]}"
    err, bound = np.abs(got - GR.reference(c, data)[0]), GR.act_bound(c, kind, data)
    ratio = float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0).max())    # an exact zero needs no bound
    print(f"gemm-range | {row} {NAME[c.prec]} {c.M}x{c.N}x{c.K} {name} | act_sweep act={act} bias={with_bias} | {GL.FAMILY[fam]} | {ratio:.3f} of the bound")
    return ratio


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("i,act", SWEEPS, ids=[f"{IDS[i]}-act{a}" for i, a in SWEEPS])
def test_activation_sweep(i, act, with_bias):
    assert sweep(i, act, with_bias) <= 1.0
