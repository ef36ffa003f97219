"""tests/gemm_layout.py on its own, no GPU: the checker of the GEMM layout tests accepts a clean strided GEMM and rejects, by name,
every fault a kernel's address code could have -- planted in a numpy emulation that computes its addresses as `row * ld + col` on
flat buffers laid out like the hook's."""
import numpy as np
import pytest
import torch

import gemm_layout as GL
from gemm_layout import Case, F32, LayoutError

# two whole 16-column tiles and a ragged one of 8; M rows well inside one guard block
BASE = Case(F32, M=20, N=40, K=32, resid=True)


@pytest.fixture(scope="module")
def clean():
    data = GL.make_data(BASE)
    return data, GL.reference(BASE, data), GL.emulate(BASE, data)


def _layouts():
    return {"dense": BASE.filled(), "strided": BASE.strided(), "window": BASE.window(), "in_place": BASE.inplace()}


def test_layouts_are_the_ones_the_issue_names():
    s, w, i = BASE.strided(), BASE.window(), BASE.inplace()
    assert (s.lda, s.ldw, s.ldc, s.ldr) == (32 + 8, 32 + 16, 40 + 24, 40 + 40) and s.c0 == 0
    assert (w.lda, w.ldw, w.ldc, w.ldr, w.c0) == (32, 32, 64, 80, 8)
    assert i.in_place and i.ldr == i.ldc == 64 and (i.lda, i.ldw) == (40, 48)
    d = BASE.filled()
    assert (d.lda, d.ldw, d.ldc, d.ldr) == (32, 32, 40, 40)
    assert GL.back_rows(300) == 212 + 8 and GL.back_rows(256) == 8 and GL.back_rows(1) == 255 + 8


@pytest.mark.parametrize("layout", ["dense", "strided", "window", "in_place"])
def test_checker_accepts_the_clean_run(clean, layout):
    data, ref, dense = clean
    launch = GL.emulate(_layouts()[layout], data)
    GL.check(launch, None if layout == "dense" else dense, ref, expect_family="tiled-vec")
    assert np.array_equal(launch.owned_bytes("out_f32"), dense.owned_bytes("out_f32"))


@pytest.mark.parametrize("fault", GL.FAULTS)
def test_checker_rejects_each_planted_fault_by_name(clean, fault):
    data, ref, dense = clean
    case = BASE.inplace() if fault == "in_place_overlap" else BASE.strided()
    launch = GL.emulate(case, data, fault)
    with_dense, alone = GL.EXPECTED_KIND[fault]
    with pytest.raises(LayoutError) as e:
        GL.check(launch, dense, ref)
    assert e.value.kind == with_dense, str(e.value)
    with pytest.raises(LayoutError) as e:
        GL.check(launch, None, ref)   # without the dense launch: the reference, the pattern and the NaN check catch it themselves
    assert e.value.kind == alone, str(e.value)


def test_the_overlapped_last_tile_is_a_fault_of_in_place_runs_only(clean):
    """the hazard the in-place layout exists for: the same kernel passes every check while the residual has a buffer of its own"""
    data, ref, dense = clean
    GL.check(GL.emulate(BASE.strided(), data, "in_place_overlap"), dense, ref)


def test_checker_rejects_another_family(clean):
    data, ref, dense = clean
    with pytest.raises(LayoutError) as e:
        GL.check(GL.emulate(BASE.strided(), data), dense, ref, expect_family="wreg")
    assert e.value.kind == "family"


def test_a_store_in_front_of_the_buffer_lands_in_the_front_guard(clean):
    data, ref, dense = clean
    launch = GL.emulate(BASE.window(), data)
    launch["out_f32"].reshape(-1)[(GL.GUARD_ROWS * launch.case.ldc - 1) * 4] ^= 1   # the element in front of row 0
    with pytest.raises(LayoutError) as e:
        GL.check(launch, dense, ref)
    assert e.value.kind == "guard"
    launch = GL.emulate(BASE.window(), data)
    launch["out_f32"][GL.GUARD_ROWS + 3, (launch.case.c0 - 1) * 4] ^= 1             # column c0 - 1 of a row: the window's left pad
    with pytest.raises(LayoutError) as e:
        GL.check(launch, dense, ref)
    assert e.value.kind == "pad"


def test_partials_checker():
    c = Case(GL.BF16, M=5, N=64, K=64, form=GL.X16, part_ld=5).filled()
    dense, wide = GL.Launch(c), GL.Launch(Case(GL.BF16, M=5, N=64, K=64, form=GL.X16, part_ld=9))
    rng = np.random.default_rng(0)
    dense.part = rng.standard_normal((2, 5, 2)).astype(np.float32)
    dense.part_guards = np.full(128, GL.SENTINEL, np.uint32).view(np.float32)
    wide.part = np.full((2, 9, 2), GL.SENTINEL, np.uint32).view(np.float32).copy()
    wide.part[:, :5] = dense.part
    wide.part_guards = dense.part_guards.copy()
    GL.check_partials(wide, dense)
    for kind, poke in (("pad", lambda: wide.part.__setitem__((1, 6, 0), 1.0)), ("dense", lambda: wide.part.__setitem__((0, 2, 1), 7.0))):
        keep = wide.part.copy()
        poke()
        with pytest.raises(LayoutError) as e:
            GL.check_partials(wide, dense)
        assert e.value.kind == kind
        wide.part = keep
    wide.part.view(np.uint32)[1, 4, 0] = GL.SENTINEL
    with pytest.raises(LayoutError):
        GL.check_partials(wide, dense)


def test_roundings_and_raw_decoders():
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(4096) * 3).astype(np.float32)
    np.testing.assert_array_equal(GL.bf16_round(a), torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy())
    # a Launch decodes each raw element type; the split type is 8 fp16 hi parts followed by 8 lo parts per group of 8 elements
    vals = (rng.standard_normal((3, 16)) * 2).astype(np.float32)
    for prec, enc in ((GL.BF16, lambda v: (v.view(np.uint32) >> 16).astype(np.uint16)), (GL.FP16, lambda v: v.astype(np.float16))):
        c = Case(prec, M=3, N=16, K=64, typed=True)
        want = GL.operand_round(prec, vals)
        L = GL.Launch(c)
        L["out_act"] = np.full((L.total_rows(), 16 * 2), 0x5A, np.uint8)
        L["out_act"][GL.GUARD_ROWS:GL.GUARD_ROWS + 3] = np.ascontiguousarray(enc(want)).view(np.uint8).reshape(3, -1)
        np.testing.assert_array_equal(L.owned("out_act"), want.astype(np.float64))
        assert L.outside_untouched("out_act") == (True, True)
    c = Case(GL.SPLIT, M=3, N=16, K=64, typed=True)
    hi = vals.astype(np.float16)
    lo = (vals - hi.astype(np.float32)).astype(np.float16)
    L = GL.Launch(c)
    L["out_act"] = np.full((L.total_rows(), 16 * 4), 0x5A, np.uint8)
    grouped = np.stack([hi.reshape(3, 2, 8), lo.reshape(3, 2, 8)], axis=2)   # [row, group, plane, 8]
    L["out_act"][GL.GUARD_ROWS:GL.GUARD_ROWS + 3] = np.ascontiguousarray(grouped).view(np.uint8).reshape(3, -1)
    np.testing.assert_array_equal(L.owned("out_act"), hi.astype(np.float64) + lo.astype(np.float64))


def test_bounds_are_the_ones_test_kernels_gpu_states():
    ref = np.array([[0.5, -4.0]])
    k = np.sqrt(512 / 64)
    assert np.allclose(GL.bound(Case(GL.BF16, 1, 2, 512), "out_f32", ref), 2e-3 * k)
    assert np.allclose(GL.bound(Case(GL.BF16, 1, 2, 512, typed=True), "out_act", ref), 2e-3 * k + np.abs(ref) * 2.0 ** -8)
    assert np.allclose(GL.bound(Case(F32, 1, 2, 512), "out_f32", ref), 2e-5 * k)
    assert np.allclose(GL.bound(Case(GL.SPLIT, 1, 2, 512), "out_f32", ref), 4e-5 * k)
    assert np.allclose(GL.bound(Case(GL.FP16, 1, 2, 512, typed=True), "out_act", ref), 3e-4 * k + 2.0 ** -10 * 4.0)
    assert np.allclose(GL.bound(Case(GL.FP16, 1, 2, 512, form=GL.X16), "out_f32", ref), np.maximum(np.abs(ref), 1) * 2.0 ** -10 + 2e-4 * k)
    assert np.allclose(GL.bound(Case(GL.BF16, 1, 2, 512, form=GL.LNF), "out_act", ref), np.maximum(np.abs(ref), 1) * 2.0 ** -8 + 6e-3)
