"""Region captions, host side (no GPU): conzic_amd/regions.py, rivals.rival_table(group_of_image=...), clip.ImageRegions against a
stub engine, the CLI flags, and the reference's own crop-equals-slice property on the boxes of the GPU tests."""
import json

import numpy as np
import pytest

import region_ref as rr
from conzic_amd import demo_cli, native, regions, rivals


# ---- regions.py ---------------------------------------------------------------------------------------------------------
def test_parse_boxes():
    assert regions.parse_boxes("1,2,3,4") == [(1, 2, 3, 4)]
    assert regions.parse_boxes(" 1, 2 ,3,4 ; 0,0,10,20;") == [(1, 2, 3, 4), (0, 0, 10, 20)]
    for bad, msg in (("", "no box given"), (";;", "no box given"), ("1,2,3", "a box is x0,y0,x1,y1"), ("1,2,3,4,5", "a box is x0,y0,x1,y1"),
                     ("1,2,3,x", "whole pixels"), ("1.5,2,3,4", "whole pixels")):
        with pytest.raises(ValueError, match=msg):
            regions.parse_boxes(bad)
    assert regions.parse_grid("2x3") == (2, 3) and regions.parse_grid("4X4") == (4, 4)
    for bad in ("2", "2x", "0x3", "axb", "2x3x4"):
        with pytest.raises(ValueError, match="grid"):
            regions.parse_grid(bad)


@pytest.mark.parametrize("w,h,rows,cols", [(131, 97, 4, 4), (131, 97, 8, 8), (10, 7, 7, 10), (5, 3, 1, 1), (1280, 960, 8, 8),
                                           (13, 11, 3, 5)])
def test_grid_covers_the_image_exactly_and_no_tile_is_empty(w, h, rows, cols):
    boxes = regions.grid_boxes(w, h, rows, cols)
    assert len(boxes) == rows * cols
    cover = np.zeros((h, w), np.int32)
    for x0, y0, x1, y1 in boxes:
        assert x0 < x1 and y0 < y1
        cover[y0:y1, x0:x1] += 1
    assert (cover == 1).all()          # every pixel in exactly one tile
    assert boxes[0][:2] == (0, 0) and boxes[-1][2:] == (w, h)
    assert boxes[1] == (w // cols, 0, 2 * w // cols, h // rows) if cols > 1 else True   # row by row
    assert regions.check_boxes(boxes, w, h) == boxes


def test_grid_refusals():
    for args, msg in (((10, 7, 8, 2), "empty tiles"), ((10, 7, 2, 11), "empty tiles"), ((10, 7, 0, 2), "at least one row"),
                      ((10, 7, 2, -1), "at least one row"), ((0, 7, 1, 1), "bad image size")):
        with pytest.raises(ValueError, match=msg):
            regions.grid_boxes(*args)


def test_check_boxes_states_the_rules_of_the_c_call():
    W, H = 131, 97
    assert regions.check_boxes([[0, 0, W, H], np.array([1, 2, 3, 4])], W, H) == [(0, 0, W, H), (1, 2, 3, 4)]
    for boxes, msg in (([], "between 1 and 1024"), ([(0, 0, 1, 1)] * 1025, "between 1 and 1024"),
                       ([(0, 0, 1, 1), (-1, 0, 5, 5)], r"box 1 = \(-1, 0, 5, 5\) leaves the 131x97 image"),
                       ([(0, -1, 5, 5)], "leaves the"), ([(0, 0, W + 1, 5)], "leaves the"), ([(0, 0, 5, H + 1)], "leaves the"),
                       ([(5, 0, 5, 5)], "is empty"), ([(0, 7, 5, 6)], "is empty"), ([(0, 0, 5)], "a box is x0,y0,x1,y1"),
                       ([(0, 0, 5, 5.5)], "whole pixels"), ([(0, 0, 5, "a")], "whole pixels")):
        with pytest.raises(ValueError, match=msg):
            regions.check_boxes(boxes, W, H)
    # the resized long side int(S * long / short): 32 * 524288 = 2^24 passes, anything above is refused
    assert regions.check_boxes([(0, 0, 524288, 1)], 600000, 1, 32)
    with pytest.raises(ValueError, match="above 2\\^24"):
        regions.check_boxes([(0, 0, 524289, 1)], 600000, 1, 32)
    assert regions.check_boxes([(0, 0, 524289, 1)], 600000, 1)     # (no S given: not checked)
    assert regions.MAX_REGIONS == native.MAX_REGIONS == 1024
    assert "czc_preprocess_regions_u8" in native.SIGNATURES and len(native.SIGNATURES["czc_preprocess_regions_u8"][1]) == 10


def test_region_name_and_regions_file(tmp_path):
    assert regions.region_name("a.jpg", (1, 2, 30, 40)) == "a.jpg#1,2,30,40"
    assert regions.region_name("a.jpg", np.array([0, 0, 5, 6])) == "a.jpg#0,0,5,6"
    with pytest.raises(ValueError):
        regions.region_name("a.jpg", (1, 2, 3))
    f = tmp_path / "r.json"
    f.write_text(json.dumps({"a.jpg": [[0, 0, 5, 6], [1, 1, 2, 2]], "b.png": [[3, 4, 5, 6]]}))
    assert regions.load_regions_file(str(f)) == {"a.jpg": [(0, 0, 5, 6), (1, 1, 2, 2)], "b.png": [(3, 4, 5, 6)]}
    for bad, msg in (([1, 2], "expected a JSON object"), ({"a.jpg": []}, "non-empty list"), ({"a.jpg": [[1, 2, 3]]}, "a box is"),
                     ({"a.jpg": [[1, 2, 3, 4.5]]}, "whole pixels"), ({"a.jpg": 5}, "non-empty list")):
        f.write_text(json.dumps(bad))
        with pytest.raises(ValueError, match=msg):
            regions.load_regions_file(str(f))


# ---- rivals.rival_table(group_of_image=...) -----------------------------------------------------------------------------
def test_rival_table_with_groups_never_crosses_groups():
    rng = np.random.default_rng(0)
    emb = rng.standard_normal((9, 16))
    groups = [0, 0, 0, 0, 1, 2, 2, 2, 2]
    t = rivals.rival_table(emb, 3, group_of_image=groups)
    assert t.shape == (9, 3) and t.dtype == np.int32
    for b in range(9):
        filled = t[b][t[b] >= 0]
        assert all(groups[j] == groups[b] and j != b for j in filled)
        assert len(filled) == min(3, groups.count(groups[b]) - 1)
    assert (t[4] == -1).all()                                        # a group of one gets no rivals
    # inside a group: the table of that group alone, re-indexed
    sub = rivals.rival_table(emb[5:], 3)
    np.testing.assert_array_equal(t[5:], np.where(sub >= 0, sub + 5, -1))
    rivals.check_table(t, np.arange(9), 9)


def test_rival_table_with_one_group_is_the_old_table():
    emb = np.random.default_rng(1).standard_normal((6, 8))
    old = rivals.rival_table(emb, 4)
    np.testing.assert_array_equal(rivals.rival_table(emb, 4, group_of_image=[7] * 6), old)
    np.testing.assert_array_equal(rivals.rival_table(emb, 4, group_of_image=None), old)
    sets = [0, 0, 0, 1, 1, 1]
    np.testing.assert_array_equal(rivals.rival_table(emb, 4, sets, group_of_image=[0] * 6), rivals.rival_table(emb, 4, sets))
    both = rivals.rival_table(emb, 4, sets, group_of_image=[0, 0, 1, 1, 2, 2])    # a rival shares set AND group
    np.testing.assert_array_equal(both[:, 0], [1, 0, -1, -1, 5, 4])
    with pytest.raises(ValueError):
        rivals.rival_table(emb, 4, group_of_image=[0] * 5)
    with pytest.raises(ValueError):
        rivals.rival_table(emb, 4, sets, group_of_image=[0] * 5)


# ---- clip.ImageRegions against a stub engine ----------------------------------------------------------------------------
class StubEngine:
    """Records the staging calls; an embedding = (slot's tag, 0...) so that order shows."""

    def __init__(self):
        self.calls, self.slots, self.resident = [], {}, None

    def preprocess_u8(self, rgb, slot=0, want_pixels=False, mean=None, std=None):
        self.calls.append(("u8", rgb.shape, slot))
        self.slots[slot] = float(rgb[0, 0, 0])

    def preprocess_regions_u8(self, rgb, boxes, slot0=0, want_pixels=False, mean=None, std=None):
        self.calls.append(("regions", rgb.shape, [tuple(b) for b in boxes], slot0))
        for i, b in enumerate(boxes):
            self.slots[slot0 + i] = float(rgb[b[1], b[0], 0]) + 1000.0

    def encode_staged(self, B):
        self.calls.append(("encode", B))
        return np.array([[self.slots[i], 0.0] for i in range(B)], dtype=np.float32)

    def encode_pil(self, images, mean=None, std=None):
        images = images if isinstance(images, (list, tuple)) else [images]
        for i, im in enumerate(images):
            self.preprocess_u8(np.asarray(im), i)
        return self.encode_staged(len(images))

    def set_image_embeds(self, e):
        self.resident = np.array(e)


def _clip(stub):
    from clip.clip import CLIP
    from conzic_amd import synth
    c = CLIP(None)
    c.czc_cfg = synth.clip_tiny(100)
    c._engine = stub
    return c


def _picture(tag, h=40, w=50):
    im = np.zeros((h, w, 3), np.uint8)
    im[..., 0] = tag + np.arange(w, dtype=np.uint8)[None, :]     # red = tag + column: a box is told by its x0
    return im


def test_image_regions_expand_in_order_and_runs_of_one_picture_share_a_call():
    from clip.clip import ImageRegions
    stub = StubEngine()
    c = _clip(stub)
    a, b, pic = _picture(200), _picture(220), _picture(0)
    boxes = [(3, 0, 10, 10), (7, 5, 20, 30), (0, 0, 50, 40)]
    out = np.asarray(c.compute_image_representation_from_image_instance([a, ImageRegions(pic, boxes), b]))
    np.testing.assert_array_equal(out[:, 0], [200, 1003, 1007, 1000, 220])      # image, its three regions in order, image
    assert stub.calls == [("u8", (40, 50, 3), 0), ("regions", (40, 50, 3), boxes, 1), ("u8", (40, 50, 3), 4), ("encode", 5)]
    # alone, and two ImageRegions of the same picture in a row: one regions call
    stub.calls.clear()
    out = np.asarray(c.compute_image_representation_from_image_instance(ImageRegions(pic, boxes[:2])))
    np.testing.assert_array_equal(out[:, 0], [1003, 1007])
    assert stub.calls == [("regions", (40, 50, 3), boxes[:2], 0), ("encode", 2)]
    stub.calls.clear()
    other = _picture(100)
    out = np.asarray(c.compute_image_representation_from_image_instance(
        [ImageRegions(pic, boxes[:1]), ImageRegions(pic, boxes[1:]), ImageRegions(other, boxes[:1])]))
    np.testing.assert_array_equal(out[:, 0], [1003, 1007, 1000, 1103])
    assert stub.calls == [("regions", (40, 50, 3), boxes, 0), ("regions", (40, 50, 3), boxes[:1], 3), ("encode", 4)]
    with pytest.raises(ValueError, match="leaves the 50x40 image"):
        c.compute_image_representation_from_image_instance(ImageRegions(pic, [(0, 0, 51, 40)]))
    with pytest.raises(ValueError):
        ImageRegions(pic, [])


def test_the_cache_key_includes_the_boxes():
    from clip.clip import ImageRegions
    stub = StubEngine()
    c = _clip(stub)
    pic = _picture(0)
    boxes = [(3, 0, 10, 10), (7, 5, 20, 30)]
    first = np.asarray(c.compute_image_representation_from_image_instance(ImageRegions(pic, boxes)))
    n = len(stub.calls)
    again = np.asarray(c.compute_image_representation_from_image_instance(ImageRegions(pic, [list(b) for b in boxes])))
    assert len(stub.calls) == n                                    # same picture, same boxes: served from the cache
    np.testing.assert_array_equal(again, first)
    np.testing.assert_array_equal(stub.resident, first)            # and made resident again
    other = np.asarray(c.compute_image_representation_from_image_instance(ImageRegions(pic, boxes[::-1])))
    assert len(stub.calls) > n                                     # other boxes (here: another order): encoded again
    np.testing.assert_array_equal(other[:, 0], [1007, 1003])
    n = len(stub.calls)
    c.compute_image_representation_from_image_instance(pic)        # the whole picture is yet another entry
    assert len(stub.calls) > n
    n = len(stub.calls)
    pic[0, 3, 0] = 99                                              # refilled in place: the fingerprint notices
    c.compute_image_representation_from_image_instance(ImageRegions(pic, boxes[::-1]))
    c.compute_image_representation_from_image_instance(ImageRegions(pic, boxes[::-1]))
    assert len(stub.calls) == n + 2                                # one regions call + one encode, then the cache


def test_without_the_device_processor_the_boxes_are_cropped_in_pil():
    import types
    from PIL import Image
    from clip.clip import ImageRegions
    stub = StubEngine()
    stub.encode_images = lambda pixels: np.asarray(pixels, dtype=np.float32).reshape(len(pixels), -1)[:, :2]
    c = _clip(stub)
    seen = []

    def processor(images, return_tensors):
        seen.extend(images)
        return {"pixel_values": np.array([[float(np.asarray(im)[0, 0, 0]), 0.0] for im in images])}
    c.processor = processor            # no .image_processor attribute: not the geometry the device implements
    assert c._device_processor_params() is None
    pic = _picture(0)
    whole = Image.fromarray(_picture(200))
    out = np.asarray(c.compute_image_representation_from_image_instance([ImageRegions(pic, [(3, 0, 10, 10), (7, 5, 20, 30)]), whole]))
    np.testing.assert_array_equal(out[:, 0], [3, 7, 200])
    assert [im.size for im in seen] == [(7, 10), (13, 25), (50, 40)]
    assert not any(call[0] == "regions" for call in stub.calls)


# ---- the reference's own property: crop(box) in PIL = the contiguous slice ----------------------------------------------
def test_crop_equals_slice_through_the_host_processor():
    from oracle.imageproc import preprocess
    im = rr.make_image()
    np.testing.assert_array_equal(rr.region_pixels(im, rr.BOXES, 32), preprocess(rr.slices(im, rr.BOXES), 32))
    np.testing.assert_array_equal(rr.region_pixels(im, rr.BOXES[:1], 32), preprocess([im], 32))   # the full frame
    regions.check_boxes(rr.BOXES, rr.W, rr.H, 32)
    big = rr.make_image(rr.H_FULL, rr.W_FULL, seed=11)
    np.testing.assert_array_equal(rr.region_pixels(big, rr.BOXES_FULL, 224), preprocess(rr.slices(big, rr.BOXES_FULL), 224))
    regions.check_boxes(rr.BOXES_FULL, rr.W_FULL, rr.H_FULL, 224)


# ---- CLI flags ----------------------------------------------------------------------------------------------------------
def test_cli_flags_default_off_and_refuse_what_the_plumbing_cannot_honour(capsys):
    a = demo_cli.get_args(["--synthetic"])
    assert a.regions is None and a.region_grid is None and a.region_full is False and a.regions_file is None
    a = demo_cli.get_args(["--synthetic", "--regions", "0,0,5,5;1,2,3,4", "--region_grid", "2x3", "--region_full", "--distinct", "1.0",
                           "--batch_samples", "--sample_tau", "0.5"])
    assert a.regions == [(0, 0, 5, 5), (1, 2, 3, 4)] and a.region_grid == (2, 3) and a.region_full
    assert demo_cli.get_args(["--synthetic", "--region_grid", "2x2"]).regions == []
    assert demo_cli.get_args(["--synthetic", "--regions_file", "r.json"]).regions_file == "r.json"
    for bad, msg in ((["--regions", "0,0,5"], "a box is x0,y0,x1,y1"), (["--region_grid", "2"], "ROWSxCOLS"),
                     (["--region_full"], "adds the whole frame"), (["--regions", "0,0,5,5", "--batch_size", "2"], "--batch_size 1"),
                     (["--regions", "0,0,5,5", "--regions_file", "r.json"], "belong to"),
                     (["--regions", "0,0,5,5", "--run_type", "retrieve", "--index_captions", "c.txt"], "--run_type retrieve"),
                     (["--regions_file", "r.json", "--run_type", "retrieve", "--index_captions", "c.txt"], "--run_type retrieve"),
                     (["--region_grid", "2x2", "--run_type", "infill", "--caption", "a _", "--order", "sequential"], "--run_type infill"),
                     (["--regions", "0,0,5,5;1,1,4,4", "--distinct", "1.0", "--rival_images", "a.jpg"], "--rival_images")):
        with pytest.raises(SystemExit):
            demo_cli.get_args(["--synthetic"] + bad)
        assert msg in capsys.readouterr().err, bad


def test_run_cli_rows_of_a_batch():
    from conzic_amd import run_cli
    assert run_cli.region_rows(["a", "b"], None) == (["a", "b"], [0, 1])
    m = {"b": [(0, 0, 5, 5), (1, 2, 3, 4)], "zz": [(0, 0, 1, 1)]}
    assert run_cli.region_rows(["a", "b", "c"], m) == (["a", "b#0,0,5,5", "b#1,2,3,4", "c"], [0, 1, 1, 2])
