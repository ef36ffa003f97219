"""-m gpu: infilling through the user layer -- runtime.run_infill (caption templates -> czc_generate_rows_from calls, one per
token length) and `--run_type infill` of the CLI."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from conzic_amd import infill, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = "Image of a"
K = 200


@pytest.fixture()
def models(monkeypatch):
    """Tiny synthetic LM / CLIP / tokenizer objects as the drop-in modules take them, on the f32 engine."""
    from clip.clip import CLIP
    from conzic_amd import runtime
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab
    from PIL import Image
    monkeypatch.setenv("CZC_PRECISION", "f32")
    monkeypatch.delenv("CZC_MEMO_ROWS", raising=False)
    sv = synth.make_vocab_tiny()
    bcfg, ccfg = synth.bert_tiny(len(sv.bert_tokens)), synth.clip_tiny(len(sv.clip_vocab))
    bt, ct = tokenizers_from_vocab(sv)
    lm = SyntheticLM(bcfg)
    clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, 12), ct)
    imgs = [Image.fromarray(u) for u in synth.make_images_u8(2, ccfg.v_image)]
    yield sv, bt, lm, clip, imgs
    runtime.evict()


def test_run_infill_in_one_batch_is_every_caption_alone(models, monkeypatch):
    """Three captions of two token lengths with unequal blank counts over two images: the given words never change, no [MASK]
    is left after the first sweep, every caption's result is that of a call on the caption alone (f32: ids identical), and
    the caller's token mask ends as after the last visited position."""
    from conzic_amd import runtime
    sv, bt, lm, clip, imgs = models
    log = logging.getLogger("infill-test")
    caps = ["the _ picture of _ _", "_ photos _", "_ picture _ the _ photo"]
    ioc = [0, 1, 1]
    names = ["img0", "img1"]
    sweeps = 3
    kw = dict(order="sequential", max_iters=sweeps, top_k=K, temperature=0.1, alpha=0.02, beta=2.0)
    parsed = [infill.parse_template(bt, PROMPT, c) for c in caps]
    assert [len(p[0]) for p in parsed] == [11, 9, 11] and [p[1] for p in parsed] == [[1, 4, 5], [0, 3], [0, 2, 4]]
    call_order = [i for members in infill.group_by_length(parsed).values() for i in members]
    assert call_order == [0, 2, 1]                               # T = 11 first (captions 0 and 2), then T = 9
    snaps = []                                                   # the ids every caption's bookkeeping was handed, in call order
    real = runtime._bookkeeping

    def spy(order, ids, cos, *a, **k):
        snaps.append((np.array(ids[:, 0]), np.array(cos[:, 0])))
        return real(order, ids, cos, *a, **k)

    monkeypatch.setattr(runtime, "_bookkeeping", spy)
    dot = bt.vocab["."]

    def fresh_mask(dot_value):
        m = synth.make_token_mask(sv)
        m[:, dot] = dot_value                                    # the engine applies the '.' rule per row itself
        m[:, bt.mask_token_id] = 0                               # a stop-word list that bans [MASK] as a word: random towers pick it
        return m

    mask = fresh_mask(0)
    got = runtime.run_infill(caps, names, lm, clip, bt, imgs, mask, PROMPT, log, image_of_caption=ioc, **kw)
    assert mask[0, dot] == 1       # the last call is caption 1's, whose last blank is position L - 1 (utils.py:53-59)
    batch = {i: snaps[n] for n, i in enumerate(call_order)}
    assert len(got) == 3 and len(snaps) == 3
    for i, (texts, scores) in enumerate(got):
        ids0, blanks, L, seed_len = parsed[i]
        ids, cos = batch[i]
        assert ids.shape == (sweeps, ids0.size)
        assert len(texts) == sweeps + 1 and len(scores) == sweeps + 1 and all(len(t) == 1 for t in texts)
        given = [c for c in range(ids0.size) if c - seed_len not in blanks]
        for s in range(sweeps):
            np.testing.assert_array_equal(ids[s, given], ids0[given])
            assert (ids[s] != bt.mask_token_id).all() and "[MASK]" not in texts[s][0]
            assert texts[s][0] == bt.decode(ids[s].tolist(), skip_special_tokens=True)
        assert scores[-1][0] == max([0] + [sc[0] for sc in scores[:-1]])
    for i in range(3):
        del snaps[:]
        m1 = fresh_mask(1 if i == 2 else 0)
        alone = runtime.run_infill([caps[i]], names, lm, clip, bt, imgs, m1, PROMPT, log, image_of_caption=[ioc[i]], **kw)
        np.testing.assert_array_equal(snaps[0][0], batch[i][0])
        np.testing.assert_allclose(snaps[0][1], batch[i][1], rtol=0, atol=1e-6)
        assert alone[0][0] == got[i][0]
        assert m1[0, dot] == (0 if i == 2 else 1)                # caption 2 ends at position 4 of 6
    # the per-row memo leaves the result alone
    monkeypatch.setenv("CZC_MEMO_ROWS", "1")
    memo = runtime.run_infill(caps, names, lm, clip, bt, imgs, fresh_mask(0), PROMPT, log, image_of_caption=ioc, **kw)
    assert [m[0] for m in memo] == [g[0] for g in got] and [m[1] for m in memo] == [g[1] for g in got]
    eng = runtime.get_engine(lm, clip, bt)
    assert eng.get_option("memo_rows") == 1
    # polish / resume: every position of every caption is visited, nothing is idle
    monkeypatch.setenv("CZC_MEMO_ROWS", "0")
    eng.profile_reset()
    drafts = [g[0][-2][0] for g in got]
    again = runtime.run_infill(drafts, names, lm, clip, bt, imgs, fresh_mask(0), PROMPT, log, image_of_caption=ioc,
                               positions="all", **dict(kw, max_iters=1))
    assert all(len(t) == 2 for t, _ in again)
    redone = [infill.parse_template(bt, PROMPT, d) for d in drafts]
    assert eng.stats()["clip_seqs"] == K * sum(p[2] for p in redone)


def test_demo_cli_infill_in_a_child_process():
    """`demo_cli --synthetic --tiny --run_type infill --caption ... --caption ...` exits 0 in a fresh process and logs a final
    and a best caption per caption."""
    caps = ["the _ picture of _", "_ photo _ _"]
    cmd = [sys.executable, "-m", "conzic_amd.demo_cli", "--synthetic", "--tiny", "--run_type", "infill", "--order", "shuffle",
           "--num_iterations", "2"]
    for c in caps:
        cmd += ["--caption", c]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = (p.stdout + p.stderr).splitlines()
    final = [ln for ln in lines if ln.startswith("final caption: ")]
    best = [ln for ln in lines if ln.startswith("best caption: ")]
    assert len(final) == len(caps) and len(best) == len(caps), lines[-20:]
    assert sum(ln.startswith("Order_list:") for ln in lines) == len(caps)
    assert "picture" in final[0] and "photo" in final[1]
