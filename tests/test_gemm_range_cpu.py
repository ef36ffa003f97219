"""The checks of tests/test_gemm_range_gpu.py can fail, and its bounds are what tests/gemm_range.py says they are (CPU only).

At every row of the GPU matrix and every construction that applies, on a sample of the elements (they do not depend on one
another; the x16 edge keeps all its special rows): the honest model gemm_range.emulate(None) lies inside E(family, precision), and
each fault that gemm_range.claims() lists for the pair lies outside 2 E on at least one element, or trips the assertions of the
x16 edge.  E itself is at most the a-priori bound of any summation order over the family's longest chain."""
from dataclasses import replace

import numpy as np
import pytest

import gemm_layout as GL
import gemm_range as GR
from gemm_range import IDS, MATRIX


def _sample(c, cname):
    rows = np.unique(np.linspace(0, c.M - 1, 24).astype(int))
    cols = np.unique(np.linspace(0, c.N - 1, 24).astype(int))
    if cname == "x16 edge":
        rows, cols = np.arange(c.M), np.arange(0, c.N, 8)
    return rows, cols


def _e(c, cname, data, ref3, fault, block):
    """max e of the modelled launch, or inf where the checker's own assertions fail"""
    rows, cols = block
    name = "out_act" if "out_f32" not in c.outputs() else "out_f32"
    out = GR.emulate(c, data, fault, block)[name]
    sub = tuple(a[np.ix_(rows, cols)] if isinstance(a, np.ndarray) else a for a in ref3)
    if cname == "x16 edge":
        try:
            return float(GR.check_x16_edge(c, data, out, sub).max())
        except AssertionError:
            return np.inf
    return float(GR.units(c, c.outputs()[name], out, sub).max())


@pytest.mark.parametrize("i", range(len(MATRIX)), ids=IDS)
def test_honest_model_is_inside_E_and_every_claimed_fault_outside_2E(i):
    _, family, c, _, fixed_k = MATRIX[i]
    key = replace(c, in_place=False, part_ld=0)
    bound = GR.row_bound(family, c)
    for cname in GR.applicable(c, fixed_k):
        data = GR.constructions(key)[cname](key, 0)
        ref3, block = GR.reference(key, data), _sample(c, cname)
        honest = _e(key, cname, data, ref3, None, block)
        assert honest <= bound, f"{IDS[i]} {cname}: the honest chain errs by {honest:.1f} units, E = {bound}"
        for fault in GR.claims(c, cname):
            e = _e(key, cname, data, ref3, fault, block)
            assert e > 2 * bound, f"{IDS[i]} {cname}: {fault} errs by {e:.1f} units only, 2 E = {2 * bound}"


def test_every_family_is_in_the_matrix_and_every_E_is_below_its_a_priori_cap():
    assert {family for _, family, _, _, _ in MATRIX} == set(GL.FAMILY.values()) - {"none"}
    pairs = {(family, c.prec) for _, family, c, _, _ in MATRIX}
    assert pairs == set(GR.E_TABLE)
    for family, prec in pairs:
        longest = max(GR.k_chain(c.prec, c.K) for _, f, c, _, _ in MATRIX if (f, c.prec) == (family, prec))
        measured, bound = GR.E_TABLE[(family, prec)]
        assert bound == int(bound) and bound >= 1 and bound == int(np.ceil(4 * measured)) and bound <= longest + 4, (family, prec, measured, bound)


def test_every_construction_separates_something():
    """no construction is in the matrix for nothing: each is claimed against at least one fault by some row (the scale pairs
    other than the unit one hold the absolute-bound hole shut: a kernel returning zeros is S / (u S) = 2^24 units out)"""
    seen = {cname.split(" in ")[0] for _, _, c, _, fixed_k in MATRIX for cname in GR.applicable(c, fixed_k) if GR.claims(c, cname)}
    assert {"scales 2 x 0.05", "outliers", "cancelling", "one-sided lo", "one-sided subnormal lo", "x16 edge"} <= seen, seen
    faults = {f for _, _, c, _, fixed_k in MATRIX for cname in GR.applicable(c, fixed_k) for f in GR.claims(c, cname)}
    assert faults == set(GR.FAULTS) - {"act_clamp"}


@pytest.mark.parametrize("prec,act,form", [(GL.BF16, 1, GL.PLAIN), (GL.FP16, 1, GL.PLAIN), (GL.F32, 1, GL.PLAIN), (GL.F32, 2, GL.PLAIN),
                                           (GL.SPLIT, 1, GL.PLAIN), (GL.SPLIT, 2, GL.PLAIN), (GL.BF16, 1, GL.LNF), (GL.FP16, 1, GL.LNF)])
@pytest.mark.parametrize("with_bias", [False, True])
def test_activation_sweep_model(prec, act, form, with_bias):
    c = GL.Case(prec, 70, 1024, 512, form=GL.LNF, act=act) if form == GL.LNF else GL.Case(prec, 16, 136, 64, act=act, typed=prec != GL.F32)
    data = GR.act_sweep(c, 0, with_bias)
    (name, kind), = c.outputs().items()
    ref = GR.reference(c, data)[0]
    pre = GR.reference(replace(c, act=0), data)[0]
    if not with_bias:   # every ceil(512 / N) consecutive rows see the whole grid -127.5 .. 127.5
        assert set((pre[:4] * 2).astype(int).ravel()) == set(range(-255, 256))
    assert all(GR.ACTS[family] for _, family, c, _, _ in MATRIX if c.form == GL.LNF), "the folded-LayerNorm family has an activation"
    out = GR.emulate(c, data)[name]
    assert np.isfinite(out).all() and (np.abs(out - ref) <= GR.act_bound(c, kind, data)).all()
    assert np.isnan(GR.emulate(c, data, "act_clamp")[name]).any()
    zeros = np.zeros_like(out)      # a kernel that skipped the activation, or returned nothing, is far outside
    assert (np.abs(zeros - ref) > GR.act_bound(c, kind, data)).any() and (np.abs(pre - ref) > GR.act_bound(c, kind, data)).any()
