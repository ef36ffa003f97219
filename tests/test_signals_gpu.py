"""-m gpu: control signals in one batch through the user layer -- runtime.caption_signals (one czc_generate_rows_hp call for all
signals, lengths and samples) and `--signals` of the CLI."""
import logging
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conzic_amd import synth
from goldutil import load_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPLATE = [["DET"], ["ADJ", "NOUN"], ["NOUN"], ["VERB"], ""]


def _objects(meta, B):  # as tests/test_lengths_gpu.py builds the synthetic models, with caller-provided control tables
    from clip.clip import CLIP
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab
    from PIL import Image
    sv = synth.make_vocab_tiny()
    bcfg, ccfg = synth.BertCfg(**meta["bert_cfg"]), synth.ClipCfg(**meta["clip_cfg"])
    bt, ct = tokenizers_from_vocab(sv)
    lm = SyntheticLM(bcfg, meta["bseed"])
    clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, meta["cseed"]), ct)
    clip.lexicon = synth.make_lexicon(len(sv.bert_tokens))
    clip.pos_tags = synth.make_pos_tags(len(sv.bert_tokens))
    imgs = [Image.fromarray(u) for u in synth.make_images_u8(B, ccfg.v_image)]
    return sv, lm, clip, bt, imgs, synth.make_token_mask(sv)


def test_caption_signals_equals_a_loop_of_the_serial_calls(monkeypatch):
    """Signals [caption, positive, negative, pos] x lengths [4, 6] x 2 samples x 2 images in one call, table mode, against
    generate_caption / control_generate_caption called serially under the same seeds (signals outside, then lengths, then
    samples), by the criterion of test_lengths_gpu.py: texts of every sweep and the best entry equal, scores to 2e-6, same RNG
    state and token mask afterwards."""
    import utils
    from conzic_amd import runtime
    from conzic_amd.engine import Engine
    from control_gen_utils import control_generate_caption
    from gen_utils import generate_caption
    monkeypatch.setenv("CZC_PRECISION", "f32")
    monkeypatch.setenv("CZC_CONTROL", "table")
    monkeypatch.delenv("CZC_MEMO_ROWS", raising=False)
    meta, _ = load_case("tiny_shuffle")
    B, S, lens = 2, 2, [4, 6]
    sigs = ["caption", "positive", "negative", "pos"]
    logger = logging.getLogger("signals-test")
    names = [f"img{j}" for j in range(B)]
    kw = dict(prompt=meta["prompt"], batch_size=B, top_k=meta["K"], temperature=meta["temperature"], max_iter=2,
              alpha=meta["alpha"], beta=meta["beta"], generate_order="shuffle")
    gamma = 0.5
    _, lm, clip, tok, imgs, mask = _objects(meta, B)
    calls = []
    real = Engine.generate_rows_hp
    monkeypatch.setattr(Engine, "generate_rows_hp", lambda self, *a, **k: (calls.append(len(a[5])), real(self, *a, **k))[1])

    def serial_call(sig, n, m):
        if sig == "caption":
            return generate_caption(names, lm, clip, tok, imgs, m, logger, max_len=n, **kw)
        return control_generate_caption(names, lm, clip, tok, imgs, m, logger, max_len=n, gamma=gamma,
                                        ctl_type="pos" if sig == "pos" else "sentiment",
                                        style_type="negative" if sig == "negative" else "positive", pos_type=TEMPLATE, **kw)

    try:
        utils.set_seed(meta["seed"])
        m1 = mask.copy()
        serial = [[[serial_call(sig, n, m1) for _ in range(S)] for n in lens] for sig in sigs]
        st_py, st_np = random.getstate(), np.random.get_state()
        assert not calls
        utils.set_seed(meta["seed"])
        m2 = mask.copy()
        got = runtime.caption_signals(sigs, lens, S, names, lm, clip, tok, imgs, m2, logger, gamma=gamma, pos_type=TEMPLATE, **kw)
        assert calls == [len(sigs) * len(lens) * S * B]       # ONE engine call, a row per signal, length, sample and image
        assert random.getstate() == st_py
        assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), st_np))
        np.testing.assert_array_equal(m1, m2)
        assert len(got) == len(sigs) and all(len(g) == len(lens) and all(len(p) == S for p in g) for g in got)
        for sig, sig_ref, sig_got in zip(sigs, serial, got):
            for per_ref, per_got in zip(sig_ref, sig_got):
                for (t_ref, s_ref), (t, s) in zip(per_ref, per_got):
                    assert t == t_ref, sig                 # every sweep's captions and the best-caption entry
                    assert [len(x) for x in s] == [len(x) for x in s_ref]
                    np.testing.assert_allclose(np.array(s), np.array(s_ref), atol=2e-6)
        finals = {sig: [t[-2] for per in g for t, _ in per] for sig, g in zip(sigs, got)}
        assert finals["positive"] != finals["negative"]     # the sign reaches the rows
    finally:
        runtime.evict()


def test_demo_cli_signals_runs_in_a_child_process():
    """`python -m conzic_amd.demo_cli --synthetic --tiny --signals caption,positive,negative` in a fresh process: exit 0 and a
    final caption per signal and sample."""
    cmd = [sys.executable, "-m", "conzic_amd.demo_cli", "--synthetic", "--tiny", "--signals", "caption,positive,negative"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = r.stdout + r.stderr
    assert log.count("final caption: ") == 3 * 2            # three signals, samples_num = 2 calls
    for sig in ("caption", "positive", "negative"):
        assert f"Signal {sig}, sentence length 10, sample 0: " in log
