"""-m gpu: option "memo_rows" of czc_generate_rows (the per-row step memo, include/conzic_hip.h, csrc/memo_rows.hip): with the
option on, a step runs only for the rows whose masked row differs from their last visit of the same key in the call, and the
call returns what it returns without the option.  Every test compares option off against option on, on the same engine; the
hit count is checked against the host statement of the rule (harness.memo_expected_hits_rows) on the option-off trajectory."""
import logging
import random

import numpy as np
import pytest

from conzic_amd import harness, native, synth
from conzic_amd.engine import Engine, EngineGroup
from goldutil import load_case

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT, REFINE = native.PREC_F32, native.PREC_BF16, native.PREC_SPLIT, native.PREC_REFINE
K = 200
ZERO = dict(hit_row_steps=0, row_steps=0)
NO_MEMO = dict(hit_image_steps=0, image_steps=0)


def _shuffles(n, L, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        o = list(range(L))
        rng.shuffle(o)
        if o not in out and o != list(range(L)):
            out.append(o)
    return out


def _shuffle_rows(R, L, sweeps, seed):
    """positions int32 [L * sweeps, R]: a different shuffle order per row."""
    cols = [harness.order_positions("shuffle", L, sweeps, order_list=o)[0] for o in _shuffles(R, L, seed)]
    return np.ascontiguousarray(np.array(cols, dtype=np.int32).T)


def _pair(eng, init, L, seed_len, pos, hp, ior=None, n_mask=None, every=1, want_cos=True, k=K):
    """The same czc_generate_rows call with the option off and on: {option: (ids, cos, stats, memo_rows_stats, memo_stats)}."""
    out = {}
    for on in (0, 1):
        eng.set_option("memo_rows", on)
        eng.profile_reset()
        ids, cos = eng.generate_rows(init, L, seed_len, k, pos, hp, image_of_row=ior, n_mask=n_mask, snapshot_every=every,
                                     want_cos=want_cos)
        out[on] = (ids, cos, eng.stats(), eng.memo_rows_stats(), eng.memo_stats())
    eng.set_option("memo_rows", 0)
    return out


def _check_hits(out, su, pos, n_mask, seed_len, T, never=None, whole_steps_only=False):
    """Engine hits == the rule on the option-off trajectory; row-steps == R x n_steps; BERT rows fall by T per row-step that
    hit an n_mask >= 1 step; czc_memo_stats stays zero.  whole_steps_only (CZC_PREC_SPLIT): only steps on which every row hits
    are skipped.  Returns the expected hit matrix."""
    n_steps, R = pos.shape
    exp = harness.memo_expected_hits_rows(out[0][0], pos, n_mask, seed_len, su.bert_tok.vocab["[MASK]"], never=never)
    if whole_steps_only:
        exp = exp & exp.all(axis=1, keepdims=True)
    print(f"[memo_rows] engine {out[1][3]}, rule {int(exp.sum())} of {exp.size}; hits per step {exp.sum(axis=1).tolist()}")
    assert out[0][3] == ZERO
    assert out[1][3] == dict(hit_row_steps=int(exp.sum()), row_steps=R * n_steps)
    assert out[0][4] == NO_MEMO and out[1][4] == NO_MEMO
    nm = np.ones(n_steps, int) if n_mask is None else np.asarray(n_mask)
    off, on = out[0][2], out[1][2]
    assert off["bert_rows"] - on["bert_rows"] == T * int(exp[nm >= 1].sum())
    if exp.any():
        assert on["clip_rows"] < off["clip_rows"] and on["bert_rows"] < off["bert_rows"]
    return exp


def test_memo_rows_option_round_trips_and_counts_nothing_when_off():
    su = harness.build_synthetic(True, F32)
    eng = su.engine
    try:
        assert eng.get_option("memo_rows") == 0            # default off
        eng.set_option("memo_rows", 1)
        assert eng.get_option("memo_rows") == 1 and eng.get_option("memo") == 0   # independent of "memo"
        r = eng.replica()
        assert r.get_option("memo_rows") == 1              # replicas inherit it
        eng.set_option("memo_rows", 0)
        assert eng.get_option("memo_rows") == 0 and r.get_option("memo_rows") == 0
        R, L = 3, 4
        eng.set_image_embeds(np.random.default_rng(0).standard_normal((R, su.clip_cfg.proj)).astype(np.float32))
        init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)
        hp = Engine.hyper(0.02, 2.0, 0.1)
        pos = _shuffle_rows(R, L, 3, 1)
        eng.set_option("memo", 1)                          # memo = 1, memo_rows = 0: a rows call as without either
        eng.profile_reset()
        ids0, cos0 = eng.generate_rows(init, L, 4, 8, pos, hp)
        assert eng.memo_rows_stats() == ZERO and eng.memo_stats() == NO_MEMO
        eng.set_option("memo", 0)
        eng.set_option("memo_rows", 1)                     # czc_generate ignores it
        eng.profile_reset()
        eng.generate(R, init, L, 4, 8, list(range(L)) * 3, hp)
        assert eng.memo_rows_stats() == ZERO and eng.memo_stats() == NO_MEMO
        eng.generate_rows(init, L, 4, 8, pos, hp)
        ms = eng.memo_rows_stats()
        assert ms["row_steps"] == R * pos.shape[0] and eng.memo_stats() == NO_MEMO
        eng.profile_reset()
        assert eng.memo_rows_stats() == ZERO               # counted since czc_profile_reset
        # a group of three steps is longer than an entry: it runs whole, never hits, and the call is what it is without the option
        pos3 = np.repeat(np.array([0, 1, 2] * 2, dtype=np.int32)[:, None], R, axis=1)
        out = _pair(eng, init, L, 4, pos3, hp, n_mask=[3, 0, 0] * 2, every=3, k=8)
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))
        assert out[1][3] == dict(hit_row_steps=0, row_steps=R * 6)
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_memo_rows_is_exact_on_a_converging_batch(prec):
    """Four images x four rows each, a different shuffle order per row, L = 6, K = 200, eight sweeps on the converging setup,
    every step snapshotted, option off against on: ids of every snapshot identical, winner cosines bit for bit
    (CZC_PREC_REFINE: its steps that return a cosine never hit, so the cosine comparison runs on a per-sweep call, within
    1e-6); the engine's hits are the rule's; some row-steps hit, and some step ran on a compact batch (CZC_PREC_SPLIT: some
    step skipped every row)."""
    B, S, L, sweeps = 4, 4, 6, 8
    R = B * S
    su, _, hp, init, seed_len = harness.converging_setup(B=B, L=L, precision=prec)
    eng = su.engine
    T = init.size
    try:
        pos = _shuffle_rows(R, L, sweeps, 5)
        ior = np.tile(np.arange(B, dtype=np.int32), S)
        if prec == REFINE:
            out = _pair(eng, init, L, seed_len, pos, hp, ior=ior, want_cos=False)
            never = harness.memo_refine_no_hit(pos.shape[0], 1, want_cos=False)
        else:
            out = _pair(eng, init, L, seed_len, pos, hp, ior=ior)
            never = None
            np.testing.assert_array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))
        np.testing.assert_array_equal(out[0][0], out[1][0])
        exp = _check_hits(out, su, pos, None, seed_len, T, never=never, whole_steps_only=prec == SPLIT)
        per_step = exp.sum(axis=1)
        assert exp.sum() > 0
        if prec == SPLIT:    # whole steps only: some step skipped every row
            assert (per_step == R).any()
        else:                # some step ran on a compact batch
            assert ((per_step > 0) & (per_step < R)).any()
        if prec == REFINE:
            o2 = _pair(eng, init, L, seed_len, pos, hp, ior=ior, every=L, want_cos=True)
            np.testing.assert_array_equal(o2[0][0], o2[1][0])
            np.testing.assert_allclose(o2[0][1], o2[1][1], rtol=0, atol=1e-6)
            assert o2[1][3]["hit_row_steps"] > 0
    finally:
        eng.close()


@pytest.fixture(scope="module")
def conv():
    """The bf16 converging setup (full-size towers), shared by the tests below; each sets the image embeds it needs."""
    B, L = 16, 6
    su, emb, hp, init, seed_len = harness.converging_setup(B=B, L=L, precision=BF16)
    yield su, emb, hp, init, seed_len, L
    su.engine.set_control_callback(None)
    su.engine.close()


@pytest.mark.parametrize("order", ["shuffle", "span"])
def test_same_order_in_every_row_is_czc_generate_with_the_memo(conv, order):
    """All rows share one order: ids, cosines and hit count of czc_generate with option "memo" on that order.  Span order
    (n_mask 2 then 0): the second step of a group hits exactly when the first did."""
    su, emb, hp, init, seed_len, L = conv
    eng = su.engine
    B, sweeps = 8, 5
    eng.set_image_embeds(emb[:B])
    pos1, nm, _ = harness.order_positions(order, L, sweeps, order_list=_shuffles(1, L, 2)[0])
    eng.set_option("memo", 1)
    eng.profile_reset()
    ids_g, cos_g = eng.generate(B, init, L, seed_len, K, pos1, hp, n_mask=nm, snapshot_every=1)
    want = eng.memo_stats()
    eng.set_option("memo", 0)
    pos = np.repeat(np.array(pos1, dtype=np.int32)[:, None], B, axis=1)
    out = _pair(eng, init, L, seed_len, pos, hp, n_mask=nm)
    for on in (0, 1):
        np.testing.assert_array_equal(out[on][0], ids_g)
        np.testing.assert_array_equal(out[on][1].view(np.int32), cos_g.view(np.int32))
    exp = _check_hits(out, su, pos, nm, seed_len, init.size)
    assert out[1][3] == dict(hit_row_steps=want["hit_image_steps"], row_steps=want["image_steps"])
    assert exp.sum() > 0
    if order == "span":
        for s in range(len(nm)):
            if nm[s] == 0:
                assert (exp[s] == exp[s - 1]).all()
        # the per-row refusal of an n_mask = 0 step behind a step that kept another row is still raised with the option on
        eng.set_option("memo_rows", 1)
        bad = np.zeros((2, B), dtype=np.int32)
        bad[1, 1] = 1
        with pytest.raises(native.NativeError, match="n_mask=0 re-use") as ei:
            eng.generate_rows(init, L, seed_len, K, bad, hp, n_mask=[1, 0], snapshot_every=2)
        assert ei.value.code == native.ERR_STATE
        eng.set_option("memo_rows", 0)


def test_span_order_on_a_compact_batch_keeps_the_reuse_rule(conv):
    """Span order with several rows per image: rows settle at different times, so n_mask = 0 steps re-use the forward of a
    compact batch, row for row."""
    su, emb, hp, init, seed_len, L = conv
    eng = su.engine
    B, S, sweeps = 4, 2, 6
    eng.set_image_embeds(emb[:B])
    pos1, nm, _ = harness.order_positions("span", L, sweeps)
    pos = np.repeat(np.array(pos1, dtype=np.int32)[:, None], B * S, axis=1)
    out = _pair(eng, init, L, seed_len, pos, hp, ior=np.repeat(np.arange(B, dtype=np.int32), S), n_mask=nm)
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))
    exp = _check_hits(out, su, pos, nm, seed_len, init.size)
    per_step = exp.sum(axis=1)
    assert ((per_step > 0) & (per_step < B * S) & (np.asarray(nm) == 0)).any()


def test_fully_converged_rows_run_nothing():
    """Rows that all reached their fixed point: the late steps take every row from its entry and run neither BERT nor the text
    tower (czc_stats counts only the steps that ran)."""
    B, S, L, sweeps = 2, 3, 6, 7
    R = B * S
    su, _, hp, init, seed_len = harness.converging_setup(B=B, L=L, precision=BF16, flat_top=0)
    eng = su.engine
    try:
        pos = _shuffle_rows(R, L, sweeps, 8)
        out = _pair(eng, init, L, seed_len, pos, hp, ior=np.tile(np.arange(B, dtype=np.int32), S))
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))
        exp = _check_hits(out, su, pos, None, seed_len, init.size)
        full = exp.all(axis=1)
        assert full[-L:].all(), exp.sum(axis=1)              # the last sweep: nothing ran
        off, on = out[0][2], out[1][2]
        assert off["steps"] == pos.shape[0] and on["steps"] == pos.shape[0] - int(full.sum())
        assert on["clip_seqs"] == off["clip_seqs"] - K * int(exp.sum())
    finally:
        eng.close()


def test_memo_rows_with_sentiment_tables_and_differing_positions(conv):
    su, emb, _, init, seed_len, L = conv
    eng = su.engine
    B, S, sweeps = 4, 3, 6
    eng.set_image_embeds(emb[:B])
    eng.set_lexicon(synth.make_lexicon(len(su.sv.bert_tokens)))
    hp = Engine.hyper(0.1, 2.0, 0.1, 0.5)
    pos = _shuffle_rows(B * S, L, sweeps, 13)
    out = _pair(eng, init, L, seed_len, pos, hp, ior=np.tile(np.arange(B, dtype=np.int32), S))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))
    exp = _check_hits(out, su, pos, None, seed_len, init.size)
    assert exp.sum() > 0


def test_memo_rows_calls_a_host_scorer_with_the_compact_batch(conv):
    """A control callback is accepted when all rows share a position per step; with the option on it is called for the rows
    that run, compacted."""
    su, emb, _, init, seed_len, L = conv
    eng = su.engine
    B, S, sweeps = 4, 3, 6
    R = B * S
    eng.set_image_embeds(emb[:B])
    lex = synth.make_lexicon(len(su.sv.bert_tokens))
    eng.set_lexicon(lex)
    hp = Engine.hyper(0.1, 2.0, 0.1, 0.5)
    pos1 = harness.order_positions("shuffle", L, sweeps, order_list=_shuffles(1, L, 4)[0])[0]
    pos = np.repeat(np.array(pos1, dtype=np.int32)[:, None], R, axis=1)
    seen = []

    def scorer(inp, cand, gen_idx):
        """A pure function of the rows: the candidate's lexicon score plus the mean score of the sentence's other words."""
        seen.append((inp.shape[0], gen_idx))
        ctx = lex[inp].mean(axis=1, keepdims=True)
        return (lex[cand] + 0.25 * ctx).astype(np.float32)

    eng.set_control_callback(scorer)
    try:
        out = _pair(eng, init, L, seed_len, pos, hp, ior=np.repeat(np.arange(B, dtype=np.int32), S))
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1].view(np.int32), out[1][1].view(np.int32))
        assert out[1][3]["hit_row_steps"] > 0
        n_off = len(pos1)
        assert [b for b, _ in seen[:n_off]] == [R] * n_off
        assert [g for _, g in seen[:n_off]] == [seed_len + p for p in pos1]
        assert min(b for b, _ in seen[n_off:]) < R
        # differing positions with a callback are still refused
        eng.set_option("memo_rows", 1)
        with pytest.raises(native.NativeError, match="control callback") as ei:
            eng.generate_rows(init, L, seed_len, K, _shuffle_rows(R, L, 1, 13), hp, image_of_row=np.repeat(np.arange(B), S))
        assert ei.value.code == native.ERR_ARG
    finally:
        eng.set_option("memo_rows", 0)
        eng.set_control_callback(None)


def test_memo_rows_on_two_streams(conv):
    """EngineGroup.generate_rows (two replicas on their own streams, each with entries of its own): ids and cosines of the
    one-stream option-off call."""
    su, emb, hp, init, seed_len, L = conv
    eng = su.engine
    B, S, sweeps = 4, 4, 6
    R = B * S
    pos = _shuffle_rows(R, L, sweeps, 17)
    ior = np.tile(np.arange(B, dtype=np.int32), S)
    eng.set_option("memo_rows", 0)
    eng.set_image_embeds(emb[:B])
    ids0, cos0 = eng.generate_rows(init, L, seed_len, K, pos, hp, image_of_row=ior, snapshot_every=L)
    grp = EngineGroup(eng, streams=2, min_images=8)
    try:
        grp.set_option("memo_rows", 1)
        assert all(e.get_option("memo_rows") == 1 for e in grp.engines)
        grp.set_image_embeds(emb[:B])
        grp.profile_reset()
        ids1, cos1 = grp.generate_rows(init, L, seed_len, K, pos, hp, image_of_row=ior, snapshot_every=L)
        np.testing.assert_array_equal(ids0, ids1)
        np.testing.assert_array_equal(cos0.view(np.int32), cos1.view(np.int32))
        ms = grp.memo_rows_stats()
        assert ms["row_steps"] == R * pos.shape[0] and ms["hit_row_steps"] > 0
        assert all(e.memo_rows_stats()["row_steps"] == R // 2 * pos.shape[0] for e in grp.engines)
        assert grp.memo_stats() == NO_MEMO
    finally:
        grp.set_option("memo_rows", 0)
        grp.close(parent=False)


@pytest.mark.parametrize("prec", [F32, SPLIT])
def test_mixed_order_goldens_with_the_option_on(prec):
    """The reference's trajectories of tests/test_rows_gpu.py (rows 0-1 full_synth_b2, shuffle; row 2 full_cfg1, sequential;
    rows 3-4 full_random, whose recorded positions revisit three columns, so those steps run the check) in one call with the
    option on."""
    m_sh, a_sh = load_case("full_synth_b2")
    m_sq, a_sq = load_case("full_cfg1")
    m_rd, a_rd = load_case("full_random")
    L, Kg = m_sh["L"], m_sh["K"]
    su = harness.build_synthetic(m_sh["tiny"], prec, m_sh["bseed"], m_sh["cseed"], m_sh["logit_scale"], m_sh["regular_only"],
                                 lexicon=m_sh["gamma"] is not None)
    eng = su.engine
    try:
        eng.set_image_embeds(np.concatenate([a_sh["image_embeds"], a_sq["image_embeds"], a_rd["image_embeds"]], axis=0))
        init = su.bert_tok.encode(m_sh["prompt"] + su.bert_tok.mask_token * L)
        cols = [m_sh["order_list"]] * 2 + [list(range(L))] + [m_rd["positions"]] * 2
        pos = np.array(cols, dtype=np.int32).T
        hp = Engine.hyper(m_sh["alpha"], m_sh["beta"], m_sh["temperature"], m_sh["gamma"], m_sh["style"] == "negative")
        eng.set_option("memo_rows", 1)
        eng.profile_reset()
        ids, cos = eng.generate_rows(init, L, 4, Kg, pos, hp, snapshot_every=10)
        ms = eng.memo_rows_stats()
        print(f"[memo_rows] goldens prec {prec}: {ms}")
        assert ms["row_steps"] == 5 * 10
        np.testing.assert_array_equal(ids[:, 0:2], a_sh["snaps"])
        np.testing.assert_array_equal(ids[:, 2:3], a_sq["snaps"][:1])
        np.testing.assert_array_equal(ids[:, 3:5], a_rd["snaps"])
        np.testing.assert_allclose(cos[:, 0:2], np.array(m_sh["scores"][:-1], dtype=np.float32), atol=2e-5)
        np.testing.assert_allclose(cos[:, 2:3], np.array(m_sq["scores"][:1], dtype=np.float32), atol=2e-5)
        np.testing.assert_allclose(cos[:, 3:5], np.array(m_rd["scores"][:-1], dtype=np.float32), atol=2e-5)
    finally:
        eng.close()


def test_caption_samples_with_czc_memo_rows(monkeypatch):
    """runtime.caption_samples (what --batch_samples of the two CLIs calls), CZC_MEMO_ROWS=1 against CZC_MEMO_ROWS=0: the same
    (texts, scores) for every sample."""
    import utils
    from clip.clip import CLIP
    from conzic_amd import runtime
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab
    from PIL import Image
    monkeypatch.setenv("CZC_PRECISION", "f32")
    monkeypatch.delenv("CZC_MEMO", raising=False)
    meta, _ = load_case("tiny_shuffle")
    B, S, L = 3, 3, 10
    res, stats = {}, {}
    for v in ("0", "1"):
        monkeypatch.setenv("CZC_MEMO_ROWS", v)
        sv = synth.make_vocab_tiny()
        bcfg, ccfg = synth.BertCfg(**meta["bert_cfg"]), synth.ClipCfg(**meta["clip_cfg"])
        bt, ct = tokenizers_from_vocab(sv)
        lm = SyntheticLM(bcfg, meta["bseed"])
        clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, meta["cseed"]), ct)
        imgs = [Image.fromarray(u) for u in synth.make_images_u8(B, ccfg.v_image)]
        try:
            utils.set_seed(meta["seed"])
            res[v] = runtime.caption_samples(S, "caption", [f"img{j}" for j in range(B)], lm, clip, bt, imgs,
                                             synth.make_token_mask(sv), logging.getLogger("memo-rows"), prompt=meta["prompt"],
                                             batch_size=B, max_len=L, top_k=meta["K"], temperature=meta["temperature"],
                                             max_iter=4, alpha=meta["alpha"], beta=meta["beta"], generate_order="shuffle")
            eng = runtime.get_engine(lm, clip, bt)
            assert eng.get_option("memo_rows") == int(v)
            stats[v] = eng.memo_rows_stats()
        finally:
            runtime.evict()
    assert stats["0"] == ZERO and stats["1"]["row_steps"] == B * S * L * 4
    assert len(res["0"]) == S
    for (t0, s0), (t1, s1) in zip(res["0"], res["1"]):
        assert t0 == t1
        assert s0 == s1
