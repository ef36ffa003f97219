"""-m gpu: czc_preprocess_regions_u8 -- N boxes of one image cropped, resized and staged in one call -- against PIL itself
(tests/region_ref.py: crop(box), then the processor) and against the single-image path on the contiguous slices.  Every
comparison is bit-exact: integer resampling restricted to the crop window, three IEEE fp32 operations per value."""
import os

import numpy as np
import pytest

import region_ref as rr
from conzic_amd import harness, native, regions, synth
from goldutil import GOLD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    su = harness.build_synthetic(True, native.PREC_F32)
    yield su
    su.engine.close()


@pytest.fixture(scope="module")
def full():
    su = harness.build_synthetic(False, native.PREC_BF16)
    yield su
    su.engine.close()


@pytest.fixture(scope="module")
def image():
    return rr.make_image()


@pytest.fixture(scope="module")
def want(image):
    """PIL's answer for rr.BOXES, computed once."""
    out = rr.region_pixels(image, rr.BOXES, 32)
    out.setflags(write=False)
    return out


def test_regions_equal_pil_and_the_single_image_path(tiny, image, want):
    eng = tiny.engine
    got = eng.preprocess_regions_u8(image, rr.BOXES, want_pixels=True)
    assert got.shape == (len(rr.BOXES), 3, 32, 32)
    for i, b in enumerate(rr.BOXES):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"box {i} {b} against PIL")
    emb = eng.encode_staged(len(rr.BOXES))   # the staged slots themselves, before the single-image path overwrites slot 0
    for i, (b, crop) in enumerate(zip(rr.BOXES, rr.slices(image, rr.BOXES))):
        one = eng.preprocess_u8(crop, slot=0, want_pixels=True)
        np.testing.assert_array_equal(got[i], one, err_msg=f"box {i} {b} against preprocess_u8 of the slice")
    np.testing.assert_array_equal(got[0], eng.preprocess_u8(image, slot=0, want_pixels=True))   # the full frame
    np.testing.assert_array_equal(emb, eng.encode_pil(rr.slices(image, rr.BOXES)))
    np.testing.assert_array_equal(emb, eng.encode_images(np.array(want)))
    np.testing.assert_array_equal(eng.encode_regions(image, rr.BOXES), emb)
    from PIL import Image
    np.testing.assert_array_equal(eng.encode_regions(Image.fromarray(image), rr.BOXES), emb)


def test_one_region(tiny, image, want):
    for i in (0, 1, 8, 9):
        got = tiny.engine.preprocess_regions_u8(image, [rr.BOXES[i]], want_pixels=True)
        np.testing.assert_array_equal(got[0], want[i])
        np.testing.assert_array_equal(tiny.engine.encode_staged(1), tiny.engine.encode_images(np.array(want[i:i + 1])))


def test_thirty_three_regions_grow_the_staged_batch_and_keep_earlier_slots(image, want):
    su = harness.build_synthetic(True, native.PREC_F32)   # a fresh engine: the staged batch starts at 8 slots
    try:
        eng = su.engine
        first = synth.make_odd_images(32)[:3]
        for i, im in enumerate(first):
            eng.preprocess_u8(im, slot=i)
        boxes = list(rr.BOXES) + regions.grid_boxes(rr.W, rr.H, 4, 4)
        assert len(boxes) == 33
        got = eng.preprocess_regions_u8(image, boxes, slot0=3, want_pixels=True)
        np.testing.assert_array_equal(got[:len(rr.BOXES)], want)
        np.testing.assert_array_equal(got, rr.region_pixels(image, boxes, 32))
        np.testing.assert_array_equal(eng.encode_staged(36), eng.encode_pil(list(first) + rr.slices(image, boxes)))
    finally:
        su.engine.close()


def test_slot0_leaves_the_slots_before_it_alone(tiny, image):
    eng = tiny.engine
    first = synth.make_odd_images(32)[:5]
    for i, im in enumerate(first):
        eng.preprocess_u8(im, slot=i)
    boxes = rr.BOXES[8:11]
    eng.preprocess_regions_u8(image, boxes, slot0=5)
    got = eng.encode_staged(8)
    np.testing.assert_array_equal(got, eng.encode_pil(list(first) + rr.slices(image, boxes)))


def test_the_chunk_size_changes_no_bit(tiny, image, want):
    eng = tiny.engine
    assert eng.get_option("regions_chunk") == 64
    try:
        for chunk in (1, 3, 64):
            eng.set_option("regions_chunk", chunk)
            assert eng.get_option("regions_chunk") == chunk
            np.testing.assert_array_equal(eng.preprocess_regions_u8(image, rr.BOXES, want_pixels=True), want, err_msg=f"chunk {chunk}")
        for bad in (0, 1025):
            with pytest.raises(native.NativeError) as exc:
                eng.set_option("regions_chunk", bad)
            assert exc.value.code == native.ERR_ARG
    finally:
        eng.set_option("regions_chunk", 64)


def test_the_order_of_the_boxes_permutes_the_slots_and_nothing_else(tiny, image, want):
    perm = np.random.default_rng(1).permutation(len(rr.BOXES))
    got = tiny.engine.preprocess_regions_u8(image, [rr.BOXES[i] for i in perm], want_pixels=True)
    np.testing.assert_array_equal(got, want[perm])


def test_a_tall_strip_costs_what_any_region_costs(tiny):
    """A one-pixel-wide box 3000 pixels tall resizes to 32 x 96000; only the rows the 32 x 32 window reads are computed."""
    im = rr.make_image(3000, 4, seed=5)
    boxes = [(2, 0, 3, 3000), (0, 100, 4, 2900)]
    got = tiny.engine.preprocess_regions_u8(im, boxes, want_pixels=True)
    np.testing.assert_array_equal(got, rr.region_pixels(im, boxes, 32))


def test_full_size_engine(full):
    eng = full.engine
    im = rr.make_image(rr.H_FULL, rr.W_FULL, seed=11)
    got = eng.preprocess_regions_u8(im, rr.BOXES_FULL, want_pixels=True)
    ref = rr.region_pixels(im, rr.BOXES_FULL, 224)
    for i, b in enumerate(rr.BOXES_FULL):
        np.testing.assert_array_equal(got[i], ref[i], err_msg=f"box {i} {b}")
    emb = eng.encode_staged(len(rr.BOXES_FULL))
    for i, crop in enumerate(rr.slices(im, rr.BOXES_FULL)):
        np.testing.assert_array_equal(got[i], eng.preprocess_u8(crop, slot=0, want_pixels=True))
    np.testing.assert_array_equal(emb, eng.encode_pil(rr.slices(im, rr.BOXES_FULL)))


@pytest.fixture
def fresh():
    su = harness.build_synthetic(True, native.PREC_F32)   # nothing staged yet: staged_n counts this test's slots only
    yield su
    su.engine.close()


def test_refusals_leave_the_staged_slots_alone(fresh, image):
    eng = fresh.engine
    H, W = rr.H, rr.W
    eng.preprocess_regions_u8(image, rr.BOXES[:4])
    before = eng.encode_staged(4)
    ok = (1, 1, 9, 9)
    cases = [
        ("no box", image, np.zeros((0, 4), np.int32), 0),
        ("too many boxes", image, [ok] * (native.MAX_REGIONS + 1), 0),
        ("negative slot0", image, [ok], -1),
        ("slot0 above 2^20", image, [ok], (1 << 20) + 1),
        ("x0 < 0", image, [ok, (-1, 0, 5, 5)], 0),
        ("y0 < 0", image, [ok, (0, -1, 5, 5)], 0),
        ("x1 > width", image, [ok, (0, 0, W + 1, 5)], 0),
        ("y1 > height", image, [ok, (0, 0, 5, H + 1)], 0),
        ("x0 >= x1", image, [ok, (5, 0, 5, 5)], 0),
        ("y0 >= y1", image, [ok, (0, 7, 5, 6)], 0),
        # 32 * 600000 / 1 > 2^24
        ("resized long side above 2^24", np.zeros((1, 600000, 3), np.uint8), [(0, 0, 600000, 1)], 0),
        # the size limit of czc_preprocess_u8: height * width <= 2^28 (the pages of the zeros are never touched)
        ("image too large", np.zeros((1, (1 << 28) + 1, 3), np.uint8), [(0, 0, 1, 1)], 0),
    ]
    for what, im, boxes, slot0 in cases:
        with pytest.raises(native.NativeError) as exc:
            eng.preprocess_regions_u8(im, boxes, slot0=slot0, want_pixels=True)
        assert exc.value.code == native.ERR_ARG, what
        assert str(exc.value), what
        np.testing.assert_array_equal(eng.encode_staged(4), before, err_msg=what)
    with pytest.raises(native.NativeError):   # staged_n is still 4
        eng.encode_staged(5)
    # exactly 2^24 is accepted: 32 * 524288 / 1
    eng.preprocess_regions_u8(np.zeros((1, 524288, 3), np.uint8), [(0, 0, 524288, 1)], slot0=4)
    eng.encode_staged(5)
    with pytest.raises(ValueError):
        eng.preprocess_regions_u8(np.zeros((4, 4), np.uint8), [ok])


@pytest.mark.parametrize("label,S", [("tiny", 32), ("full", 224)])
def test_the_single_image_path_keeps_its_golden_bits_after_a_regions_call(tiny, full, label, S):
    eng = (tiny if S == 32 else full).engine
    im = rr.make_image(200, 150, seed=9)
    eng.preprocess_regions_u8(im, regions.grid_boxes(150, 200, 2, 3) + [(0, 0, 150, 200)])
    z = np.load(os.path.join(GOLD, f"imageproc_{label}.npz"))
    imgs = synth.make_odd_images(S)[: int(z["n"])]
    gold = synth.pixels_from_u8(z["crops"])
    for i, one in enumerate(imgs):
        np.testing.assert_array_equal(eng.preprocess_u8(one, slot=i, want_pixels=True), gold[i], err_msg=f"image {i} {one.shape}")
