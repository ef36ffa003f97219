"""-m gpu: what a call leaves behind in the engine.  A step takes its batch -- rows, image rows, per-row records -- and its mode
as arguments (csrc/engine.hip StepArgs), so nothing a call sets up for its steps outlives it: a step that fails in the middle of a
compact batch leaves the resident images and the records of later calls alone, and czc_step does not inherit czc_generate's mode.
Both tests compare bytes against a second engine, built the same way, that did not go through the first call."""
import numpy as np
import pytest

from conzic_amd import harness, native, synth
from conzic_amd.engine import Engine

pytestmark = pytest.mark.gpu
F32, REFINE = native.PREC_F32, native.PREC_REFINE
K = 8
N_HOT, FLAT_TOP = 6, 4


def _converging_tiny(prec):
    """harness.converging_setup on the tiny towers: N_HOT regular tokens far above a bulk that softmax(logits / 0.1) sends to zero,
    the first FLAT_TOP of them level, so the CLIP term (published logit scale x100) picks among them image by image and the rows
    of one image settle a sweep or so before the other's: steps in between run on a compact batch.
    Two resident images.  Returns (setup, image embeds [2, proj], prompt, seed_len)."""
    sv = harness.cached_vocab(True)
    bcfg = synth.bert_tiny(len(sv.bert_tokens))
    w = synth.make_bert_weights(bcfg, 11)
    regular = np.nonzero(synth.make_token_mask(sv, regular_only=True)[0] > 0)[0]
    hot = np.random.default_rng(5).choice(regular, size=N_HOT, replace=False)
    lift = np.linspace(16.0, 5.6, N_HOT).astype(np.float32)
    lift[:FLAT_TOP] = 16.0
    bias = w["cls.predictions.bias"].copy()
    bias[hot] += lift
    w["cls.predictions.bias"] = bias
    if "cls.predictions.decoder.bias" in w:
        w["cls.predictions.decoder.bias"] = bias
    su = harness.build_synthetic(True, prec, logit_scale=4.6052, regular_only=True, bert_w=w, bert_cfg=bcfg)
    emb = np.random.default_rng(100).standard_normal((2, su.clip_cfg.proj)).astype(np.float32)
    su.engine.set_image_embeds(emb)
    prompt = "Image of a"
    return su, emb, prompt, len(prompt.split()) + 1


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def test_a_failed_compact_batch_step_leaves_the_engine_as_it_found_it():
    """Option "memo_rows" on, two resident images, four rows over them (image_of_row 1 0 1 0), L = 4, K = 8, six sweeps of one
    shuffle order with a host scorer that raises the first time it is handed fewer than four rows -- inside the step of a
    compact batch, which runs on its own rows, image rows and records.  The call fails with the scorer's exception.  Then, with
    the scorer removed, czc_generate on the two resident images, a czc_generate_rows_vs call over the same image_of_row and
    czc_score_rows return the bytes they return on an engine that never failed."""
    L, R, sweeps = 4, 4, 6
    ior = np.array([1, 0, 1, 0], dtype=np.int32)
    hp_ctl = Engine.hyper(0.02, 2.0, 0.1, 0.5)
    hp = Engine.hyper(0.02, 2.0, 0.1)
    lex = synth.make_lexicon(len(harness.cached_vocab(True).bert_tokens))
    pos1 = harness.order_positions("shuffle", L, sweeps, order_list=[2, 0, 3, 1])[0]
    pos = np.repeat(np.array(pos1, dtype=np.int32)[:, None], R, axis=1)
    rivals = np.array([[0], [1], [0], [1]], dtype=np.int32)     # the other resident image
    deltas = np.array([0.5, 1.0, 0.5, 2.0], dtype=np.float32)

    def build():
        su, _, prompt, seed_len = _converging_tiny(F32)
        su.engine.set_option("memo_rows", 1)
        init = np.array(su.bert_tok.encode(prompt + su.bert_tok.mask_token * L), dtype=np.int32)
        return su, init, seed_len

    def after(su, init, seed_len):
        eng = su.engine
        ids_g, cos_g = eng.generate(2, init, L, seed_len, K, pos1, hp, snapshot_every=1)
        start = np.repeat(init[None, :], R, axis=0)
        ids_v, cos_v = eng.generate_rows_vs(start, None, seed_len, K, pos, [hp] * R, None, None, rivals, deltas, image_of_row=ior,
                                            snapshot_every=1)
        cos_s = eng.score_rows(ids_v[-1], seed_len, image_of_row=ior)
        return ids_g, cos_g, ids_v, cos_v, cos_s

    failed, init, seed_len = build()
    clean, _, _ = build()
    try:
        seen = []

        def scorer(inp, cand, gen_idx):
            seen.append(inp.shape[0])
            if inp.shape[0] < R:
                raise KeyError("scorer failed on a compact batch")
            ctx = lex[inp].mean(axis=1, keepdims=True)
            return (lex[cand] + 0.25 * ctx).astype(np.float32)

        failed.engine.set_control_callback(scorer)
        with pytest.raises(KeyError, match="scorer failed on a compact batch"):
            failed.engine.generate_rows(init, L, seed_len, K, pos, hp_ctl, image_of_row=ior, snapshot_every=1)
        failed.engine.set_control_callback(None)
        print(f"[engine_state] rows handed to the scorer, step by step: {seen}")
        assert seen[0] == R and 0 < seen[-1] < R and all(n == R for n in seen[:-1])
        got, want = after(failed, init, seed_len), after(clean, init, seed_len)
        for name, g, w in zip(("generate ids", "generate cos", "rows_vs ids", "rows_vs cos", "score_rows cos"), got, want):
            assert _bits(g).tobytes() == _bits(w).tobytes(), name
        assert np.isfinite(got[1]).all() and np.isfinite(got[3]).all() and np.isfinite(got[4]).all()
    finally:
        failed.engine.set_control_callback(None)
        failed.engine.close()
        clean.engine.close()


def test_mode_flags_are_not_sticky():
    """CZC_PREC_REFINE, tiny towers, two images, K = 8: czc_generate selects with its own threshold, strata and margin gate;
    czc_step returns all K scores and uses none of them.  One czc_step right after a two-sweep czc_generate returns the ids,
    probabilities and all K clip / final scores, byte for byte, of the same czc_step on a fresh engine."""
    L = 4
    hp = Engine.hyper(0.02, 2.0, 0.1)
    want = ("probs", "idxs", "cand_ids", "clip_score", "clip_ref", "final_score", "best", "best_cos")

    def one_step(generate_first):
        su, _, prompt, seed_len = _converging_tiny(REFINE)
        eng = su.engine
        try:
            init = np.array(su.bert_tok.encode(prompt + su.bert_tok.mask_token * L), dtype=np.int32)
            if generate_first:
                ids, cos = eng.generate(2, init, L, seed_len, K, list(range(L)) * 2, hp)
                assert ids.shape == (2, 2, init.size) and np.isfinite(cos).all()
            inp = np.ascontiguousarray(np.repeat(init[None, :], 2, axis=0))
            res = eng.step(inp, seed_len, K, hp, want=want)
            assert (inp[:, seed_len] != su.bert_tok.vocab["[MASK]"]).all()   # the winner was written back
            res["inp"] = inp
            return res
        finally:
            eng.close()

    fresh, used = one_step(False), one_step(True)
    for name in want + ("inp",):
        assert _bits(used[name]).tobytes() == _bits(fresh[name]).tobytes(), name
    assert np.isfinite(fresh["final_score"]).all()
