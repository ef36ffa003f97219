"""-m gpu: rival images through the runtime and the CLIs (runtime.run_generation / run_generation_samples on
czc_generate_rows_vs; --distinct of the CLIs; EngineGroup.generate_rows_vs).  Tiny synthetic towers, three images."""
import logging

import numpy as np
import pytest

from conzic_amd import harness, lengths, native, rivals, synth
from conzic_amd.engine import Engine, EngineGroup

pytestmark = pytest.mark.gpu
BASE = ["--synthetic", "--tiny", "--run_type", "caption", "--batch_size", "3", "--sentence_len", "5", "--num_iterations", "2",
        "--candidate_k", "50"]
OWN = "P(own image | caption) among 3 images: "


def _run(argv, caplog):
    from conzic_amd import demo_cli, runtime
    caplog.clear()
    try:
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            demo_cli.main(argv)
    finally:
        runtime.evict()
    return [r.getMessage() for r in caplog.records]


def _objects(logit_scale=2.6592, B=3):
    from PIL import Image
    from clip.clip import CLIP
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab
    sv = synth.make_vocab_tiny()
    bcfg, ccfg = synth.bert_tiny(len(sv.bert_tokens)), synth.clip_tiny(len(sv.clip_vocab))
    ccfg.logit_scale = logit_scale
    bt, ct = tokenizers_from_vocab(sv)
    clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, 12), ct)
    imgs = [Image.fromarray(u) for u in synth.make_images_u8(B, ccfg.v_image)]
    return SyntheticLM(bcfg), clip, bt, imgs, synth.make_token_mask(sv)


class Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def _generate(monkeypatch, prec, logit_scale, **kw):
    import utils
    from conzic_amd import runtime
    if prec is None:
        monkeypatch.delenv("CZC_PRECISION", raising=False)
    else:
        monkeypatch.setenv("CZC_PRECISION", prec)
    lm, clip, tok, imgs, mask = _objects(logit_scale)
    utils.set_seed(7)
    log = Log()
    try:
        out = runtime.run_generation("sequential", ["a", "b", "c"], lm, clip, tok, imgs, mask, "Image of a", log, 5, 50, 0.1, 0.02, 2.0,
                                     2, 3, **kw)
    finally:
        runtime.evict()
    return out, log.lines


def test_run_generation_logs_the_probability_of_the_own_image(monkeypatch):
    (texts0, _), lines0 = _generate(monkeypatch, "f32", 2.6592)
    (texts1, scores1), lines1 = _generate(monkeypatch, "f32", 2.6592, rivals=2, delta=2.0)
    assert not any(OWN in ln for ln in lines0)
    own = [ln for ln in lines1 if OWN in ln]
    assert len(own) == 3 and all(0.0 <= float(ln.rsplit(": ", 1)[1]) <= 1.0 for ln in own)
    assert len(texts1) == 3 and len(scores1) == 3            # two sweeps + best, as without rivals
    assert texts0 != texts1                                   # the term acts
    (texts2, _), lines2 = _generate(monkeypatch, "f32", 2.6592, rivals=2, delta=0.0)
    assert texts2 == texts0 and not any(OWN in ln for ln in lines2)   # delta 0: the existing call
    table = np.array([[1, -1], [2, 0], [0, 1]], dtype=np.int32)       # a hand-made table: image 0 against image 1 only
    _, lines3 = _generate(monkeypatch, "f32", 2.6592, rivals=table, delta=2.0)
    assert sum("among 2 images" in ln for ln in lines3) == 1 and sum(OWN in ln for ln in lines3) == 2


@pytest.mark.parametrize("extra", [[], ["--sample_tau", "0.5"], ["--run_type", "controllable"]])
def test_the_sample_loop_equals_the_batched_call(extra, monkeypatch, caplog):
    monkeypatch.setenv("CZC_PRECISION", "bf16")
    monkeypatch.setenv("CZC_CONTROL", "table")
    monkeypatch.delenv("CZC_MEMO_ROWS", raising=False)
    argv = BASE + ["--order", "shuffle", "--samples_num", "3", "--distinct", "1.5", "--distinct_rivals", "2"] + extra
    out = {}
    for tag, more in (("loop", []), ("batched", ["--batch_samples"])):
        msgs = _run(argv + more, caplog)
        out[tag] = ([m for m in msgs if m.startswith("final caption: ")], sorted(m for m in msgs if OWN in m))
        assert len(out[tag][0]) == 9 and len(out[tag][1]) == 9
    assert out["loop"] == out["batched"]
    if "--sample_tau" not in extra:
        # the term acts: without --distinct the argmax picks other words.  (Under --sample_tau 0.5 on these towers the Gumbel
        # noise among the few candidates BERT leaves eligible outweighs 1.5 x the spread of disc, and the captions stay: the
        # drawn path is held to the term by tests/test_rival_kernel_gpu.py::test_skipped_term_keeps_the_bits.)
        off = [m for m in _run(BASE + ["--order", "shuffle", "--samples_num", "3"] + extra, caplog) if m.startswith("final caption: ")]
        assert off != out["loop"][0]


@pytest.fixture()
def standin():  # tests/nltk_standin.py as `nltk`: the exact control mode (host scorer called back per step) without nltk
    import sys
    import nltk_standin
    saved = {k: sys.modules.get(k) for k in ("nltk", "nltk.tokenize", "nltk.corpus")}
    m = nltk_standin.install()
    yield m
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def test_controllable_run_with_the_exact_scorer(standin, monkeypatch):
    """The reference's sentence scorer called back per step serves a rivals call too: the batch rides as rows at one shared
    position per step, which is what the callback is told."""
    monkeypatch.delenv("CZC_CONTROL", raising=False)   # auto -> exact where nltk imports
    (texts0, _), lines0 = _generate(monkeypatch, "f32", 2.6592, gamma=5.0, ctl_signal="positive")
    (texts1, _), lines1 = _generate(monkeypatch, "f32", 2.6592, gamma=5.0, ctl_signal="positive", rivals=2, delta=2.0)
    assert any(ln == "control scores: exact" for ln in lines0) and any(ln == "control scores: exact" for ln in lines1)
    assert sum(OWN in ln for ln in lines1) == 3 and len(texts1) == 3
    (texts2, _), _ = _generate(monkeypatch, "f32", 2.6592, gamma=5.0, ctl_signal="positive", rivals=2, delta=0.0)
    assert texts2 == texts0


def test_rival_only_images_of_the_demo(tmp_path, monkeypatch, caplog):
    from PIL import Image
    monkeypatch.setenv("CZC_PRECISION", "bf16")
    files = []
    for i, u in enumerate(synth.make_images_u8(5, 32)[3:]):
        files.append(str(tmp_path / f"rival{i}.png"))
        Image.fromarray(u).save(files[-1])
    msgs = _run(["--synthetic", "--tiny", "--run_type", "caption", "--order", "sequential", "--samples_num", "1", "--sentence_len", "5",
                 "--num_iterations", "2", "--candidate_k", "50", "--distinct", "1.0", "--rival_images", ",".join(files)], caplog)
    assert sum(OWN in m for m in msgs) == 1 and sum(m.startswith("final caption: ") for m in msgs) == 1


def test_two_streams_equal_one_engine():
    su = harness.build_synthetic(True, native.PREC_BF16)
    eng = su.engine
    grp = None
    try:
        lens = [3, 6, 4, 6, 1, 5, 2, 6]
        ior = np.array([0, 1, 2, 0, 1, 2, 0, 1], dtype=np.int32)
        emb = np.random.default_rng(3).standard_normal((3, su.clip_cfg.proj)).astype(np.float32)
        start = lengths.length_rows(su.bert_tok, "Image of a", lens)
        pos, _, _ = lengths.length_schedules(lens, "sequential", 2)
        hps = [Engine.hyper(0.02, 2.0, 0.1) for _ in lens]
        tab = rivals.expand(rivals.rival_table(emb, 2), ior)
        dl = np.array([1.0, 0.0, 0.5, 2.0, 1.0, 0.0, 0.5, 1.0], dtype=np.float32)
        eng.set_image_embeds(emb)
        ids0, cos0 = eng.generate_rows_vs(start, lens, 4, 200, pos, hps, None, None, tab, dl, image_of_row=ior)
        grp = EngineGroup(eng, streams=2, min_images=2)
        assert len(grp.parts(len(lens))) == 2
        grp.set_image_embeds(emb)
        ids1, cos1 = grp.generate_rows_vs(start, lens, 4, 200, pos, hps, None, None, tab, dl, image_of_row=ior)
        np.testing.assert_array_equal(ids0, ids1)
        np.testing.assert_array_equal(cos0.view(np.int32), cos1.view(np.int32))
    finally:
        if grp is not None:
            grp.close(parent=False)
        eng.close()


def test_the_refine_engine_hands_the_call_to_the_split_engine(monkeypatch):
    """logit_scale = ln 100 selects the screen-then-refine engine; a call with rivals says so and runs on the split-fp16 one:
    the captions of CZC_PRECISION=split."""
    (texts, _), lines = _generate(monkeypatch, None, 4.6052, rivals=2, delta=2.0)
    assert any("screen-then-refine" in ln and ln.startswith("engine precision") for ln in lines)
    assert sum("runs on the split-fp16 engine" in ln for ln in lines) == 1
    assert sum(OWN in ln for ln in lines) == 3
    (want, _), _ = _generate(monkeypatch, "split", 4.6052, rivals=2, delta=2.0)
    assert texts == want
