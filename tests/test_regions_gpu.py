"""-m gpu: region captions through the drop-in CLIP wrapper and the two CLIs (clip.ImageRegions; demo_cli --regions /
--region_grid / --region_full; run_cli --regions_file).  Tiny synthetic towers."""
import json
import logging
import os

import numpy as np
import pytest

import region_ref as rr
from conzic_amd import harness, native, regions, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clip_and_engine():
    from clip.clip import CLIP
    su = harness.build_synthetic(True, native.PREC_F32)
    c = CLIP(None)
    c.czc_cfg = su.clip_cfg
    c._engine = su.engine
    yield c, su.engine
    su.engine.close()


def test_clip_with_image_regions_returns_the_embeddings_of_the_host_crops(clip_and_engine):
    from PIL import Image
    from clip.clip import ImageRegions
    c, eng = clip_and_engine
    im = rr.make_image()
    want = eng.encode_pil(rr.slices(im, rr.BOXES))
    got = np.asarray(c.compute_image_representation_from_image_instance(ImageRegions(im, rr.BOXES)))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(c.last_image_embeds(), want)
    got = np.asarray(c.compute_image_representation_from_image_instance(ImageRegions(Image.fromarray(im), rr.BOXES)))
    np.testing.assert_array_equal(got, want)


def test_a_mixed_list_keeps_its_order(clip_and_engine):
    from clip.clip import ImageRegions
    c, eng = clip_and_engine
    im = rr.make_image()
    a, b = synth.make_odd_images(32)[:2]
    boxes = rr.BOXES[8:12]
    want = eng.encode_pil([a] + rr.slices(im, boxes) + [b])
    got = np.asarray(c.compute_image_representation_from_image_instance([a, ImageRegions(im, boxes), b]))
    np.testing.assert_array_equal(got, want)


def test_the_cache_serves_the_same_boxes_and_encodes_other_boxes(clip_and_engine, monkeypatch):
    from clip.clip import ImageRegions
    c, eng = clip_and_engine
    im = rr.make_image(seed=4)
    calls = []
    real = eng.preprocess_regions_u8
    monkeypatch.setattr(eng, "preprocess_regions_u8", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    first = np.asarray(c.compute_image_representation_from_image_instance(ImageRegions(im, rr.BOXES[:3])))
    again = np.asarray(c.compute_image_representation_from_image_instance(ImageRegions(im, rr.BOXES[:3])))
    assert len(calls) == 1
    np.testing.assert_array_equal(again, first)
    other = np.asarray(c.compute_image_representation_from_image_instance(ImageRegions(im, rr.BOXES[1:4])))
    assert len(calls) == 2
    np.testing.assert_array_equal(other, eng.encode_pil(rr.slices(im, rr.BOXES[1:4])))


def _demo(argv, caplog):
    from conzic_amd import demo_cli, runtime
    caplog.clear()
    try:
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            finals = demo_cli.main(argv)
    finally:
        runtime.evict()
    return finals, [r.getMessage() for r in caplog.records]


DEMO = ["--synthetic", "--tiny", "--run_type", "caption", "--samples_num", "1", "--sentence_len", "5", "--num_iterations", "2",
        "--candidate_k", "50"]


def test_demo_cli_region_grid_captions_the_four_host_crops(monkeypatch, caplog):
    monkeypatch.setenv("CZC_PRECISION", "f32")
    pic = synth.make_images_u8(1, 32)[0]
    boxes = regions.grid_boxes(32, 32, 2, 2)
    finals, lines = _demo(DEMO + ["--region_grid", "2x2"], caplog)
    assert len(finals) == 4 and all(len(f) == 1 for f in finals)
    for b in boxes:   # the log line that names an image names its box
        assert any(regions.region_name("img0", b) in ln for ln in lines), b
    real = synth.make_images_u8
    monkeypatch.setattr(synth, "make_images_u8", lambda n, s, *a, **k: rr.slices(pic, boxes) if n == 4 else real(n, s, *a, **k))
    crops, _ = _demo(DEMO + ["--batch_size", "4"], caplog)
    assert finals == crops
    # --region_full puts the whole frame first; --regions follow the grid
    monkeypatch.setattr(synth, "make_images_u8", real)
    more, lines = _demo(DEMO + ["--region_grid", "1x2", "--region_full", "--regions", "3,4,20,30"], caplog)
    assert len(more) == 4
    names = [regions.region_name("img0", b) for b in [(0, 0, 32, 32), (0, 0, 16, 32), (16, 0, 32, 32), (3, 4, 20, 30)]]
    firsts = [next(i for i, ln in enumerate(lines) if n in ln) for n in names]
    assert firsts == sorted(firsts)
    with pytest.raises(SystemExit, match="leaves the 32x32 image"):
        _demo(DEMO + ["--regions", "0,0,33,5"], caplog)


@pytest.mark.parametrize("extra", [["--batch_samples", "--sample_tau", "0.5", "--samples_num", "2"], ["--distinct", "1.0"],
                                   ["--sentence_lens", "4,6"], ["--signals", "caption,positive"], ["--block_width", "2"],
                                   ["--fluency"]])
def test_demo_cli_regions_are_the_images_of_the_batch_for_the_other_flags(monkeypatch, caplog, extra):
    monkeypatch.setenv("CZC_PRECISION", "f32")
    _, lines = _demo(DEMO + ["--order", "sequential", "--region_grid", "1x2", "--region_full"] + extra, caplog)
    for b in [(0, 0, 32, 32), (0, 0, 16, 32), (16, 0, 32, 32)]:
        assert any(regions.region_name("img0", b) in ln for ln in lines), (extra, b)
    if "--distinct" in extra:
        assert sum("P(own image | caption) among 3 images" in ln for ln in lines) >= 3


def _pictures(tmp_path, n=4, size=40):
    from PIL import Image
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    for j, u in enumerate(synth.make_images_u8(n, size)):
        Image.fromarray(u).save(img_dir / f"im{j}.png")
    return img_dir, os.listdir(img_dir)


def _run_cli(tmp_path, monkeypatch, tag, argv):
    from conzic_amd import run_cli, runtime
    out_dir = tmp_path / tag
    out_dir.mkdir()
    monkeypatch.chdir(out_dir)
    try:
        run_cli.main(argv)
    finally:
        runtime.evict()
    files = {}
    for root, _, fs in os.walk(out_dir / "results"):
        for f in fs:
            files[os.path.relpath(os.path.join(root, f), out_dir)] = json.load(open(os.path.join(root, f)))
    return files


RUN = ["--synthetic", "--tiny", "--batch_size", "2", "--samples_num", "1", "--run_type", "caption", "--order", "sequential",
       "--sentence_len", "5", "--candidate_k", "50", "--num_iterations", "2"]


def test_run_cli_regions_file_keys_and_untouched_images(tmp_path, monkeypatch):
    monkeypatch.setenv("CZC_PRECISION", "f32")
    img_dir, names = _pictures(tmp_path)
    # the first batch's pictures have entries, the second batch's have none
    rmap = {names[0]: [[0, 0, 20, 20], [10, 5, 40, 40]], names[1]: [[0, 0, 40, 40], [5, 5, 6, 30], [20, 0, 40, 20]]}
    rfile = tmp_path / "regions.json"
    rfile.write_text(json.dumps(rmap))
    base = RUN + ["--caption_img_path", str(img_dir)]
    today = _run_cli(tmp_path, monkeypatch, "today", base)
    got = _run_cli(tmp_path, monkeypatch, "regions", base + ["--regions_file", str(rfile)])
    assert set(got) == set(today) and len(got) == 3
    keys = [regions.region_name(n, b) for n in names[:2] for b in rmap[n]]
    for f, content in got.items():
        assert list(content) == keys + names[2:], f
        for n in names[2:]:   # an image without an entry: what it produces today
            assert content[n] == today[f][n], (f, n)


@pytest.mark.parametrize("extra", [["--batch_samples", "--samples_num", "2", "--sample_tau", "0.5"], ["--sentence_lens", "4,6"],
                                   ["--signals", "caption,positive"], ["--block_width", "2"]])
def test_run_cli_regions_file_under_the_other_batch_paths(tmp_path, monkeypatch, extra):
    monkeypatch.setenv("CZC_PRECISION", "f32")
    img_dir, names = _pictures(tmp_path, n=2)
    rmap = {names[1]: [[0, 0, 20, 20], [10, 5, 40, 40]]}
    rfile = tmp_path / "regions.json"
    rfile.write_text(json.dumps(rmap))
    got = _run_cli(tmp_path, monkeypatch, "out", RUN + ["--caption_img_path", str(img_dir), "--regions_file", str(rfile)] + extra)
    keys = [names[0]] + [regions.region_name(names[1], b) for b in rmap[names[1]]]
    assert got and all(list(content) == keys for content in got.values()), extra


def test_run_cli_distinct_scopes_the_rivals_to_the_picture(tmp_path, monkeypatch):
    from conzic_amd import runtime
    monkeypatch.setenv("CZC_PRECISION", "f32")
    img_dir, names = _pictures(tmp_path, n=2)
    rmap = {names[0]: [[0, 0, 20, 20], [10, 5, 40, 40]], names[1]: [[0, 0, 40, 40], [5, 5, 6, 30], [20, 0, 40, 20]]}
    rfile = tmp_path / "regions.json"
    rfile.write_text(json.dumps(rmap))
    tables = []
    real = runtime._rival_call

    def spy(*a, **k):
        vs = real(*a, **k)
        tables.append(None if vs is None else np.array(vs["table"]))
        return vs
    monkeypatch.setattr(runtime, "_rival_call", spy)
    got = _run_cli(tmp_path, monkeypatch, "distinct", RUN + ["--caption_img_path", str(img_dir), "--regions_file", str(rfile),
                                                              "--distinct", "1.0", "--distinct_rivals", "4"])
    assert len(got) == 3 and all(len(v) == 5 for v in got.values())
    assert len(tables) == 1 and tables[0] is not None
    t, groups = tables[0], [0, 0, 1, 1, 1]
    assert t.shape[0] == 5
    for r in range(5):
        filled = [int(j) for j in t[r] if j >= 0]
        assert filled and all(groups[j] == groups[r] and j != r for j in filled), (r, t[r])
        assert len(filled) == groups.count(groups[r]) - 1
