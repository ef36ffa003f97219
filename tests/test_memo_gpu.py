"""-m gpu: option "memo" of czc_generate (the exact step memo, include/conzic_hip.h, csrc/memo.hip): with the option on, a step
runs only for the images whose masked row differs from their last visit of the same key in the call, and the call returns
what it returns without the option.  The hit count is checked against the host statement of the rule
(harness.memo_expected_hits) on the memo-off trajectory."""
import logging
import sys

import numpy as np
import pytest

from conzic_amd import harness, native, synth
from conzic_amd.engine import Engine, EngineGroup
from goldutil import load_case

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT, REFINE = native.PREC_F32, native.PREC_BF16, native.PREC_SPLIT, native.PREC_REFINE
K = 200


def _pair(eng, B, init, L, seed_len, positions, hp, n_mask=None, every=1, want_cos=True):
    """The same czc_generate call with the memo off and on: {memo: (ids, cos, stats, memo_stats)}."""
    out = {}
    for memo in (0, 1):
        eng.set_option("memo", memo)
        eng.profile_reset()
        ids, cos = eng.generate(B, init, L, seed_len, K, positions, hp, n_mask=n_mask, snapshot_every=every, want_cos=want_cos)
        out[memo] = (ids, cos, eng.stats(), eng.memo_stats())
    eng.set_option("memo", 0)
    return out


def _check_hits(out, su, positions, n_mask, seed_len, B, T, never=None, whole_steps_only=False):
    """Engine hits == the rule on the memo-off trajectory; BERT rows fall by T per image-step that hit an n_mask >= 1 step.
    whole_steps_only (CZC_PREC_SPLIT): only steps on which every image hits are skipped.  Returns the expected hit matrix."""
    mask_id = su.bert_tok.vocab["[MASK]"]
    exp = harness.memo_expected_hits(out[0][0], positions, n_mask, seed_len, mask_id, never=never)
    if whole_steps_only:
        exp = exp & exp.all(axis=1, keepdims=True)
    off, on = out[0][2], out[1][2]
    assert out[0][3] == dict(hit_image_steps=0, image_steps=0)
    assert out[1][3] == dict(hit_image_steps=int(exp.sum()), image_steps=B * len(positions))
    nm = np.ones(len(positions), int) if n_mask is None else np.asarray(n_mask)
    assert off["bert_rows"] - on["bert_rows"] == T * int(exp[nm >= 1].sum())
    if exp.any():
        assert on["clip_rows"] < off["clip_rows"] and on["bert_rows"] < off["bert_rows"]
    return exp


def test_memo_option_round_trips_and_counts_nothing_when_off():
    su = harness.build_synthetic(True, F32)
    eng = su.engine
    try:
        assert eng.get_option("memo") == 0                 # default off
        eng.set_option("memo", 1)                          # accepted after czc_finalize_weights (bench.py --opt)
        assert eng.get_option("memo") == 1
        r = eng.replica()
        assert r.get_option("memo") == 1                   # replicas inherit it
        eng.set_option("memo", 0)
        assert eng.get_option("memo") == 0 and r.get_option("memo") == 0
        B, L = 2, 4
        eng.set_image_embeds(np.random.default_rng(0).standard_normal((B, su.clip_cfg.proj)).astype(np.float32))
        init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)
        eng.profile_reset()
        eng.generate(B, init, L, 4, 8, list(range(L)) * 3, Engine.hyper(0.02, 2.0, 0.1))
        assert eng.memo_stats() == dict(hit_image_steps=0, image_steps=0)
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_memo_is_exact_on_a_converging_batch(prec):
    """B = 16, L = 6, K = 200, six sequential sweeps on the converging setup, every step snapshotted, memo off against on:
    the ids of every snapshot identical and the winner cosines bit for bit (CZC_PREC_REFINE: its steps that return a cosine
    never hit, so the cosine comparison runs on a per-sweep call, within 1e-6); the engine's hits are the rule's; at least 30 %
    of the image-steps of sweeps 3-6 hit and some step ran on a compact batch (0 < B_act < B; CZC_PREC_SPLIT skips whole steps
    only)."""
    B, L, sweeps = 16, 6, 6
    su, _, hp, init, seed_len = harness.converging_setup(B=B, L=L, precision=prec)
    eng = su.engine
    T = init.size
    try:
        pos = list(range(L)) * sweeps
        if prec == REFINE:
            out = _pair(eng, B, init, L, seed_len, pos, hp, every=1, want_cos=False)
            never = harness.memo_refine_no_hit(len(pos), 1, want_cos=False)
        else:
            out = _pair(eng, B, init, L, seed_len, pos, hp, every=1)
            never = None
            np.testing.assert_array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))
        np.testing.assert_array_equal(out[0][0], out[1][0])
        exp = _check_hits(out, su, pos, None, seed_len, B, T, never=never, whole_steps_only=prec == SPLIT)
        rule = harness.memo_expected_hits(out[0][0], pos, None, seed_len, su.bert_tok.vocab["[MASK]"], never=never)
        late = rule[2 * L:]   # what the rule lets hit (CZC_PREC_SPLIT takes the whole steps of it)
        assert late.mean() >= 0.30, late.mean()
        per_step = exp.sum(axis=1)
        if prec == SPLIT:    # whole steps only: some step skipped every image
            assert (per_step == B).any()
        else:                # some step ran on a compact batch
            assert ((per_step > 0) & (per_step < B)).any()
        print(f"[memo] prec {prec}: hits {int(exp.sum())} of {exp.size} image-steps, sweeps 3-6 {late.mean():.2f}; "
              f"bert_rows {out[1][2]['bert_rows']} / {out[0][2]['bert_rows']}, clip_rows {out[1][2]['clip_rows']} / {out[0][2]['clip_rows']}")
        if prec == REFINE:
            o2 = _pair(eng, B, init, L, seed_len, pos, hp, every=L, want_cos=True)
            np.testing.assert_array_equal(o2[0][0], o2[1][0])
            np.testing.assert_allclose(o2[0][1], o2[1][1], rtol=0, atol=1e-6)
            assert o2[1][3]["hit_image_steps"] > 0
    finally:
        eng.close()


@pytest.mark.parametrize("order", ["shuffle", "span", "random"])
def test_memo_is_exact_in_every_order(order):
    B, L, sweeps = 16, 6, 6
    su, _, hp, init, seed_len = harness.converging_setup(B=B, L=L, precision=BF16)
    eng = su.engine
    T = init.size
    try:
        rng = np.random.default_rng(7)
        if order == "random":
            pos, nm = [int(p) for p in rng.integers(0, L, size=L * sweeps)], [1] * (L * sweeps)
        else:
            pos, nm, _ = harness.order_positions(order, L, sweeps, order_list=list(rng.permutation(L)))
        out = _pair(eng, B, init, L, seed_len, pos, hp, n_mask=nm, every=1)
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))
        exp = _check_hits(out, su, pos, nm, seed_len, B, T)
        assert exp.sum() > 0
        if order == "span":   # the n_mask = 0 step goes with its n_mask = 2 step
            for s in range(len(pos)):
                if nm[s] == 0:
                    assert (exp[s] == exp[s - 1]).all()
    finally:
        eng.close()


def test_fully_converged_steps_run_nothing():
    """A batch whose every image reached its fixed point: the late steps take every image from the memo (B_act = 0) and run
    neither BERT nor the text tower (czc_stats counts only the steps that ran)."""
    B, L, sweeps = 4, 6, 6
    su, _, hp, init, seed_len = harness.converging_setup(B=B, L=L, precision=BF16, flat_top=0)
    eng = su.engine
    T = init.size
    try:
        pos = list(range(L)) * sweeps
        out = _pair(eng, B, init, L, seed_len, pos, hp, every=1)
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))
        exp = _check_hits(out, su, pos, None, seed_len, B, T)
        full = exp.all(axis=1)
        assert full[-L:].all(), exp.sum(axis=1)              # the last sweep: nothing ran
        off, on = out[0][2], out[1][2]
        assert off["steps"] == len(pos) and on["steps"] == len(pos) - int(full.sum())
        assert on["clip_seqs"] == off["clip_seqs"] - K * int(exp.sum())
    finally:
        eng.close()


def test_memo_with_sentiment_tables_and_a_host_scorer():
    """Sentiment control from the lexicon tables and from a host callback: results identical with the memo on, and the
    callback was called with the compact batch (B < 16) on some step."""
    B, L, sweeps = 16, 6, 5
    su, _, _, init, seed_len = harness.converging_setup(B=B, L=L, precision=BF16)
    eng = su.engine
    try:
        lex = synth.make_lexicon(len(su.sv.bert_tokens))
        eng.set_lexicon(lex)
        hp = Engine.hyper(0.1, 2.0, 0.1, 0.5)
        pos = list(range(L)) * sweeps
        out = _pair(eng, B, init, L, seed_len, pos, hp, every=1)
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))
        assert out[1][3]["hit_image_steps"] > 0
        seen = []

        def scorer(inp, cand, gen_idx):
            """A pure function of the rows: the candidate's lexicon score plus the mean score of the sentence's other words."""
            seen.append(inp.shape[0])
            ctx = lex[inp].mean(axis=1, keepdims=True)
            return (lex[cand] + 0.25 * ctx).astype(np.float32)

        eng.set_control_callback(scorer)
        out2 = _pair(eng, B, init, L, seed_len, pos, hp, every=1)
        np.testing.assert_array_equal(out2[0][0], out2[1][0])
        np.testing.assert_array_equal(out2[0][1].view(np.int32), out2[1][1].view(np.int32))
        assert out2[1][3]["hit_image_steps"] > 0
        n_off = len(pos)
        assert all(b == B for b in seen[:n_off])
        assert min(seen[n_off:]) < B
    finally:
        eng.set_control_callback(None)
        eng.close()


def test_memo_on_two_streams():
    """EngineGroup (two replicas on their own streams, each with its memo): ids and cosines of the one-stream memo-off call."""
    B, L, sweeps = 64, 6, 5
    su, emb, hp, init, seed_len = harness.converging_setup(B=B, L=L, precision=BF16)
    eng = su.engine
    grp = EngineGroup(eng, streams=2, min_images=32)
    try:
        pos = list(range(L)) * sweeps
        eng.set_option("memo", 0)
        ids0, cos0 = eng.generate(B, init, L, seed_len, K, pos, hp, snapshot_every=L)
        grp.set_option("memo", 1)
        assert all(e.get_option("memo") == 1 for e in grp.engines)
        grp.set_image_embeds(emb)
        grp.profile_reset()
        ids1, cos1 = grp.generate(B, init, L, seed_len, K, pos, hp, snapshot_every=L)
        np.testing.assert_array_equal(ids0, ids1)
        np.testing.assert_array_equal(cos0.view(np.int32), cos1.view(np.int32))
        ms = grp.memo_stats()
        assert ms["image_steps"] == B * len(pos) and ms["hit_image_steps"] > 0
        per = [e.memo_stats()["hit_image_steps"] for e in grp.engines]
        print(f"[memo] two streams: hits per stream {per} of {B // 2 * len(pos)} image-steps each")
    finally:
        grp.close(parent=True)


def _dropin_objects(meta):
    from clip.clip import CLIP
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab
    sv = harness.cached_vocab(meta["tiny"] if "tiny" in meta else True)
    bcfg = synth.BertCfg(**meta["bert_cfg"])
    ccfg = synth.ClipCfg(**meta["clip_cfg"])
    bt, ct = tokenizers_from_vocab(sv)
    lm = SyntheticLM(bcfg, meta["bseed"])
    clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, meta["cseed"]), ct)
    from PIL import Image
    imgs = [Image.fromarray(u) for u in synth.make_images_u8(meta["B"], ccfg.v_image)]
    return lm, clip, bt, imgs, synth.make_token_mask(sv), sv


def test_dropin_generate_caption_with_czc_memo(monkeypatch):
    """gen_utils.generate_caption as demo.py calls it, CZC_MEMO=1 against CZC_MEMO=0: the same (texts, scores)."""
    import utils
    from conzic_amd import runtime
    from gen_utils import generate_caption
    meta, _ = load_case("tiny_seq")
    monkeypatch.setenv("CZC_PRECISION", "f32")
    res = {}
    for memo in ("0", "1"):
        monkeypatch.setenv("CZC_MEMO", memo)
        lm, clip, tok, imgs, mask, _ = _dropin_objects(meta)
        utils.set_seed(meta["seed"])
        kw = dict(prompt=meta["prompt"], batch_size=meta["B"], max_len=meta["L"], top_k=meta["K"],
                  temperature=meta["temperature"], max_iter=3 * meta["L"], alpha=meta["alpha"], beta=meta["beta"],
                  generate_order="sequential")
        res[memo] = generate_caption([f"img{j}" for j in range(meta["B"])], lm, clip, tok, imgs, mask, logging.getLogger("memo"), **kw)
        eng = runtime.get_engine(lm, clip, tok)
        assert eng.get_option("memo") == int(memo)
        runtime.evict()
    assert res["0"][0] == res["1"][0]
    assert res["0"][1] == res["1"][1]


def test_full_size_golden_with_the_memo_on(monkeypatch):
    """The reference's own full-size trajectory (control_generate_caption, sentiment, shuffle order, the context-dependent
    scorer called back per step) still comes out with CZC_MEMO=1, as tests/test_control_gpu.py asserts it without the memo.
    Random-weight towers rarely reach a fixed point, so this shows the option does no harm on the reference's data."""
    import nltk_standin
    import utils
    from conzic_amd import runtime
    from control_gen_utils import control_generate_caption
    saved = {k: sys.modules.get(k) for k in ("nltk", "nltk.tokenize", "nltk.corpus")}
    nltk_standin.install()
    try:
        monkeypatch.setenv("CZC_PRECISION", "f32")
        monkeypatch.setenv("CZC_MEMO", "1")
        monkeypatch.delenv("CZC_CONTROL", raising=False)
        meta, _ = load_case("full_senti_shuffle_neg_ctx")
        lm, clip, tok, imgs, mask, _ = _dropin_objects(meta)
        utils.set_seed(meta["seed"])
        kw = dict(prompt=meta["prompt"], batch_size=meta["B"], max_len=meta["L"], top_k=meta["K"],
                  temperature=meta["temperature"], max_iter=meta["I"], alpha=meta["alpha"], beta=meta["beta"],
                  gamma=meta["gamma"], generate_order=meta["order"], ctl_type="sentiment", style_type=meta["style"])
        texts, scores = control_generate_caption([f"img{j}" for j in range(meta["B"])], lm, clip, tok, imgs, mask,
                                                 logging.getLogger("memo"), **kw)
        assert texts == meta["texts"]
        np.testing.assert_allclose(np.array(scores, dtype=np.float64), np.array(meta["scores"]), atol=2e-5)
        eng = runtime.get_engine(lm, clip, tok)
        assert eng.get_option("memo") == 1
        ms = eng.memo_stats()
        print(f"[memo] full-size golden: {ms['hit_image_steps']} of {ms['image_steps']} image-steps hit")
        runtime.evict()
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
