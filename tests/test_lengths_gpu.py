"""-m gpu: mixed sentence lengths through the user layer -- runtime.caption_lengths (one czc_generate_rows_len call for all
lengths and samples), `--sentence_lens` of the CLI, and runtime.run_infill with captions of several token lengths in one call."""
import logging
import random

import numpy as np
import pytest

from conzic_amd import infill, synth
from goldutil import load_case

pytestmark = pytest.mark.gpu
PROMPT = "Image of a"


def _objects(meta, B):  # as tests/test_rows_gpu.py builds the synthetic models
    from clip.clip import CLIP
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab
    from PIL import Image
    sv = synth.make_vocab_tiny()
    bcfg, ccfg = synth.BertCfg(**meta["bert_cfg"]), synth.ClipCfg(**meta["clip_cfg"])
    bt, ct = tokenizers_from_vocab(sv)
    lm = SyntheticLM(bcfg, meta["bseed"])
    clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, meta["cseed"]), ct)
    imgs = [Image.fromarray(u) for u in synth.make_images_u8(B, ccfg.v_image)]
    return sv, lm, clip, bt, imgs, synth.make_token_mask(sv)


def test_caption_lengths_equals_a_loop_of_generate_caption_per_length(monkeypatch):
    """Lengths [4, 7, 10] x 2 samples x 2 images in one call against generate_caption per length and sample (lengths outside,
    samples inside), by the criterion of test_rows_gpu.py::test_run_generation_samples_equals_the_serial_sample_loop: texts of
    every sweep and the best entry equal, scores to 2e-6, same RNG state and token mask afterwards."""
    import utils
    from conzic_amd import runtime
    from conzic_amd.engine import Engine
    from gen_utils import generate_caption
    monkeypatch.setenv("CZC_PRECISION", "f32")
    monkeypatch.delenv("CZC_MEMO_ROWS", raising=False)
    meta, _ = load_case("tiny_shuffle")
    B, S, lens = 2, 2, [4, 7, 10]
    logger = logging.getLogger("lengths-test")
    names = [f"img{j}" for j in range(B)]
    kw = dict(prompt=meta["prompt"], batch_size=B, top_k=meta["K"], temperature=meta["temperature"], max_iter=2,
              alpha=meta["alpha"], beta=meta["beta"], generate_order="shuffle")
    _, lm, clip, tok, imgs, mask = _objects(meta, B)
    calls = []
    real = Engine.generate_rows_len
    monkeypatch.setattr(Engine, "generate_rows_len", lambda self, *a, **k: (calls.append(np.asarray(a[1]).tolist()), real(self, *a, **k))[1])
    try:
        utils.set_seed(meta["seed"])
        m1 = mask.copy()
        serial = [[generate_caption(names, lm, clip, tok, imgs, m1, logger, max_len=n, **kw) for _ in range(S)] for n in lens]
        st_py, st_np = random.getstate(), np.random.get_state()
        assert not calls
        utils.set_seed(meta["seed"])
        m2 = mask.copy()
        got = runtime.caption_lengths(lens, S, "caption", names, lm, clip, tok, imgs, m2, logger, **kw)
        assert calls == [[n for n in lens for _ in range(S * B)]]       # ONE engine call, a row per length, sample and image
        assert random.getstate() == st_py
        assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), st_np))
        np.testing.assert_array_equal(m1, m2)
        assert len(got) == len(lens) and all(len(g) == S for g in got)
        for per_ref, per_got in zip(serial, got):
            for (t_ref, s_ref), (t, s) in zip(per_ref, per_got):
                assert t == t_ref                      # every sweep's captions and the best-caption entry
                assert [len(x) for x in s] == [len(x) for x in s_ref]
                np.testing.assert_allclose(np.array(s), np.array(s_ref), atol=2e-6)
        assert len({tuple(t[-2]) for t, _ in got[-1]}) > 1  # the samples took different orders to different captions
    finally:
        runtime.evict()


def test_demo_cli_sentence_lens_prints_one_caption_per_length(caplog):
    """`demo_cli --synthetic --sentence_lens 4,6`: every sample is one call and logs a final and a best caption per length; with
    --batch_samples one call serves all samples and logs the same number of captions."""
    from conzic_amd import demo_cli, runtime
    argv = ["--synthetic", "--tiny", "--order", "shuffle", "--sentence_lens", "4,6", "--num_iterations", "2", "--control_scores", "table"]
    out = []
    for extra in ([], ["--batch_samples"]):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            demo_cli.main(argv + extra)
        out.append([r.getMessage() for r in caplog.records])
        runtime.evict()
    for msgs in out:
        heads = [m for m in msgs if m.startswith("Sentence length ")]
        assert sorted(heads) == sorted(f"Sentence length {n}, sample {s}: " for n in (4, 6) for s in ((0, 1) if msgs is out[1] else (0, 0)))
        assert sum(m.startswith("final caption: ") for m in msgs) == 4 and sum(m.startswith("best caption: ") for m in msgs) == 4
        orders = [eval(m[len("Order_list:"):]) for m in msgs if m.startswith("Order_list:")]
        assert sorted(len(o) for o in orders) == [4, 4, 6, 6] and all(sorted(o) == list(range(len(o))) for o in orders)
        assert not any("one call at a time" in m for m in msgs)


def test_run_infill_with_two_token_lengths_is_one_call_with_the_two_calls_results(monkeypatch):
    """Captions of token lengths 11, 9, 11 over two images: run_infill makes ONE czc_generate_rows_len call and returns, caption
    for caption, what one run_infill call per token length returns (each of those is one czc_generate_rows_from call, as before
    the lengths call existed).  Texts of every sweep equal; scores to 1e-6, the bound of tests/test_infill_gpu.py where only the
    BERT row count differs; the token mask ends as after the last length's call."""
    from conzic_amd import runtime
    from conzic_amd.engine import Engine
    monkeypatch.setenv("CZC_PRECISION", "f32")
    monkeypatch.delenv("CZC_MEMO_ROWS", raising=False)
    meta, _ = load_case("tiny_shuffle")
    sv, lm, clip, bt, imgs, _ = _objects(meta, 2)
    log = logging.getLogger("lengths-test")
    caps = ["the _ picture of _ _", "_ photos _", "_ picture _ the _ photo"]
    ioc, names = [0, 1, 1], ["img0", "img1"]
    kw = dict(order="sequential", max_iters=3, top_k=200, temperature=0.1, alpha=0.02, beta=2.0)
    parsed = [infill.parse_template(bt, PROMPT, c) for c in caps]
    groups = infill.group_by_length(parsed)
    assert list(groups.items()) == [(11, [0, 2]), (9, [1])]
    counts = {"len": 0, "from": 0}
    real_len, real_from = Engine.generate_rows_len, Engine.generate_rows_from

    def count(kind, real):
        def wrapped(self, *a, **k):
            counts[kind] += 1
            return real(self, *a, **k)
        return wrapped

    monkeypatch.setattr(Engine, "generate_rows_len", count("len", real_len))
    monkeypatch.setattr(Engine, "generate_rows_from", count("from", real_from))

    def fresh_mask():
        m = synth.make_token_mask(sv)
        m[:, bt.vocab["."]] = 0
        m[:, bt.mask_token_id] = 0                               # random towers would pick [MASK] as a word
        return m

    try:
        m1 = fresh_mask()
        got = runtime.run_infill(caps, names, lm, clip, bt, imgs, m1, PROMPT, log, image_of_caption=ioc, **kw)
        assert counts == {"len": 1, "from": 0}
        m2 = fresh_mask()
        want = [None] * len(caps)
        for members in groups.values():
            part = runtime.run_infill([caps[i] for i in members], names, lm, clip, bt, imgs, m2, PROMPT, log,
                                      image_of_caption=[ioc[i] for i in members], **kw)
            for i, res in zip(members, part):
                want[i] = res
        assert counts == {"len": 1, "from": 2}
        np.testing.assert_array_equal(m1, m2)
        for (t, s), (t_ref, s_ref) in zip(got, want):
            assert t == t_ref and len(t) == kw["max_iters"] + 1
            np.testing.assert_allclose(np.array(s), np.array(s_ref), rtol=0, atol=1e-6)
    finally:
        runtime.evict()


def test_run_cli_sentence_lens_writes_the_files_of_a_run_per_length(monkeypatch, tmp_path):
    """run_cli --run_type caption --order sequential, 2 batches x 2 samples: `--sentence_lens 3,5` (with and without
    --batch_samples) writes, per length, the files that a `--sentence_len` run at that length writes, with the same captions."""
    import json
    import os
    from PIL import Image
    from conzic_amd import run_cli, runtime
    monkeypatch.setenv("CZC_PRECISION", "f32")
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    for j, u in enumerate(synth.make_images_u8(4, 40)):
        Image.fromarray(u).save(img_dir / f"im{j}.png")
    base = ["--synthetic", "--tiny", "--caption_img_path", str(img_dir), "--batch_size", "2", "--samples_num", "2", "--run_type", "caption",
            "--order", "sequential", "--candidate_k", "12", "--num_iterations", "2"]
    outs = []
    for name, runs in (("serial", [["--sentence_len", "3"], ["--sentence_len", "5"]]), ("lens", [["--sentence_lens", "3,5"]]),
                       ("lens_rows", [["--sentence_lens", "3,5", "--batch_samples"]])):
        out_dir = tmp_path / name
        out_dir.mkdir()
        monkeypatch.chdir(out_dir)
        for extra in runs:
            run_cli.main(base + extra)
            runtime.evict()
        files = {}
        for root, _, fs in os.walk(out_dir / "results"):
            for f in fs:
                files[os.path.relpath(os.path.join(root, f), out_dir)] = json.load(open(os.path.join(root, f)))
        outs.append(files)
    assert len(outs[0]) == 2 * 2 * 3 and {k.split("_")[2] for k in outs[0]} == {"len3", "len5"}
    for got in outs[1:]:
        assert set(got) == set(outs[0])
        for k in outs[0]:
            assert len(got[k]) == 4 and got[k] == outs[0][k], k
