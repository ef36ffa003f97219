"""czc_generate_rows: every row of a batch carries its own visiting order and names its image.

Pinned by the reference through goldens that differ only in their visiting order (mixed in one call), and against the engine
itself: a rows call equals one czc_generate call per order, row for row."""
import logging
import random

import numpy as np
import pytest

from conzic_amd import harness, native, synth
from conzic_amd.engine import Engine, EngineGroup
from goldutil import load_case

pytestmark = pytest.mark.gpu
SEED_LEN = 4
BF16, F32, SPLIT, REFINE = native.PREC_BF16, native.PREC_F32, native.PREC_SPLIT, native.PREC_REFINE


def _setup(meta, prec):  # as tests/test_streams_gpu.py builds a golden's engine
    su = harness.build_synthetic(meta["tiny"], prec, meta["bseed"], meta["cseed"], meta["logit_scale"], meta["regular_only"],
                                 lexicon=meta["gamma"] is not None)
    if meta.get("pos"):
        su.engine.set_pos(synth.make_pos_tags(len(su.sv.bert_tokens)), synth.pos_template_masks(meta["pos"]))
    return su


def _hyper(meta):
    return Engine.hyper(meta["alpha"], meta["beta"], meta["temperature"], meta["gamma"], meta["style"] == "negative",
                        control="pos" if meta.get("pos") else None)


def _shuffles(n, L, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        o = list(range(L))
        rng.shuffle(o)
        if o not in out and o != list(range(L)):
            out.append(o)
    return out


def _cos_equal(prec, got, want):
    if prec == SPLIT:  # split-fp16 kernels are chosen by row count (tests/test_streams_gpu.py): fp32-level differences remain
        np.testing.assert_allclose(got, want, atol=2e-6)
    else:
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("prec", [F32, SPLIT])
def test_mixed_orders_reproduce_three_goldens_in_one_call(prec):
    """Rows 0-1 full_synth_b2 (shuffle), row 2 full_cfg1 (sequential), rows 3-4 full_random (its recorded positions): one call,
    ten steps, one snapshot."""
    m_sh, a_sh = load_case("full_synth_b2")
    m_sq, a_sq = load_case("full_cfg1")
    m_rd, a_rd = load_case("full_random")
    for m in (m_sq, m_rd):
        assert all(m[k] == m_sh[k] for k in ("bseed", "cseed", "regular_only", "K", "L", "alpha", "beta", "temperature", "logit_scale"))
    L, K = m_sh["L"], m_sh["K"]
    su = _setup(m_sh, prec)
    try:
        su.engine.set_image_embeds(np.concatenate([a_sh["image_embeds"], a_sq["image_embeds"], a_rd["image_embeds"]], axis=0))
        init = su.bert_tok.encode(m_sh["prompt"] + su.bert_tok.mask_token * L)
        cols = [m_sh["order_list"]] * 2 + [list(range(L))] + [m_rd["positions"]] * 2
        assert cols[0] == [7, 3, 2, 8, 5, 6, 9, 4, 0, 1] and cols[3] == [6, 3, 7, 4, 6, 9, 2, 6, 7, 4]
        pos = np.array(cols, dtype=np.int32).T
        ids, cos = su.engine.generate_rows(init, L, SEED_LEN, K, pos, _hyper(m_sh), snapshot_every=10)
        assert ids.shape == (1, 5, len(init))
        np.testing.assert_array_equal(ids[:, 0:2], a_sh["snaps"])
        np.testing.assert_array_equal(ids[:, 2:3], a_sq["snaps"][:1])
        np.testing.assert_array_equal(ids[:, 3:5], a_rd["snaps"])
        np.testing.assert_allclose(cos[:, 0:2], np.array(m_sh["scores"][:-1], dtype=np.float32), atol=2e-5)
        np.testing.assert_allclose(cos[:, 2:3], np.array(m_sq["scores"][:1], dtype=np.float32), atol=2e-5)
        np.testing.assert_allclose(cos[:, 3:5], np.array(m_rd["scores"][:-1], dtype=np.float32), atol=2e-5)
    finally:
        su.engine.close()


@pytest.mark.parametrize("name,prec", [("tiny_senti_shuffle", F32), ("tiny_senti_seq", F32), ("full_pos", SPLIT)])
def test_mixed_orders_with_table_control(name, prec):
    """A control golden mixed with itself: rows 0-1 its two images under the golden's order, rows 2-3 the same images under
    another order (sequential for the shuffle golden, a shuffle for the sequential ones).  Bridge control scores, repeat count,
    POS slot and write-back all depend on the row's own column."""
    meta, arr = load_case(name)
    L, K, I = meta["L"], meta["K"], meta["I"]
    su = _setup(meta, prec)
    try:
        hp = _hyper(meta)
        init = su.bert_tok.encode(meta["prompt"] + su.bert_tok.mask_token * L)
        gold, nm, every = harness.order_positions(meta["order"], L, I, order_list=meta["order_list"])
        assert gold == meta["positions"]
        other_list = list(range(L)) if meta["order"] == "shuffle" else _shuffles(1, L, 3)[0]
        other, _, _ = harness.order_positions("shuffle", L, I, order_list=other_list)
        su.engine.set_image_embeds(arr["image_embeds"])
        ref_ids, ref_cos = su.engine.generate(2, init, L, SEED_LEN, K, other, hp, n_mask=nm, snapshot_every=every)
        pos = np.array([gold, gold, other, other], dtype=np.int32).T
        ids, cos = su.engine.generate_rows(init, L, SEED_LEN, K, pos, hp, image_of_row=[0, 1, 0, 1], n_mask=nm, snapshot_every=every)
        np.testing.assert_array_equal(ids[:, 0:2], arr["snaps"])
        np.testing.assert_allclose(cos[:, 0:2], np.array(meta["scores"][:-1], dtype=np.float32), atol=2e-5)
        np.testing.assert_array_equal(ids[:, 2:4], ref_ids)
        _cos_equal(prec, cos[:, 2:4], ref_cos)
        assert not np.array_equal(ids[:, 2:4], ids[:, 0:2])  # the other order does lead somewhere else
    finally:
        su.engine.close()


def _random_setup(prec, B):
    su = harness.build_synthetic(False, prec, logit_scale=2.6592 if prec == BF16 else 4.6052, regular_only=True)
    emb = np.random.default_rng(7).standard_normal((B, su.clip_cfg.proj)).astype(np.float32)
    return su, emb


@pytest.mark.parametrize("prec", [BF16, SPLIT, REFINE, F32])
def test_same_order_in_every_row_is_czc_generate(prec):
    B, L, K, I = 9, 6, 64, 2
    su, emb = _random_setup(prec, B)
    try:
        eng = su.engine
        eng.set_image_embeds(emb)
        init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)
        hp = Engine.hyper(0.02, 2.0, 0.1)
        for order_list in (None, _shuffles(1, L, 1)[0]):
            pos, nm, every = harness.order_positions("shuffle" if order_list else "sequential", L, I, order_list=order_list)
            ids0, cos0 = eng.generate(B, init, L, SEED_LEN, K, pos, hp, n_mask=nm, snapshot_every=every)
            rows = np.repeat(np.array(pos, dtype=np.int32)[:, None], B, axis=1)
            ids, cos = eng.generate_rows(init, L, SEED_LEN, K, rows, hp, n_mask=nm, snapshot_every=every)
            np.testing.assert_array_equal(ids, ids0)
            np.testing.assert_array_equal(cos, cos0)
            ids, cos = eng.generate_rows(init, L, SEED_LEN, K, rows, hp, image_of_row=np.arange(B), n_mask=nm, snapshot_every=every)
            np.testing.assert_array_equal(ids, ids0)
            np.testing.assert_array_equal(cos, cos0)
        eng.set_option("memo", 1)
        eng.profile_reset()
        ids, cos = eng.generate_rows(init, L, SEED_LEN, K, rows, hp, n_mask=nm, snapshot_every=every)
        np.testing.assert_array_equal(ids, ids0)
        np.testing.assert_array_equal(cos, cos0)
        assert eng.memo_stats() == dict(hit_image_steps=0, image_steps=0)
    finally:
        su.engine.close()


def test_span_order_in_every_row_is_czc_generate():
    """n_mask = 2 then 0: the re-use of the forward holds per row."""
    B, L, K = 3, 6, 32
    su, emb = _random_setup(BF16, B)
    try:
        su.engine.set_image_embeds(emb)
        init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)
        hp = Engine.hyper(0.02, 2.0, 0.1)
        pos, nm, every = harness.order_positions("span", L, 1)
        ids0, cos0 = su.engine.generate(B, init, L, SEED_LEN, K, pos, hp, n_mask=nm, snapshot_every=every)
        rows = np.repeat(np.array(pos, dtype=np.int32)[:, None], B, axis=1)
        ids, cos = su.engine.generate_rows(init, L, SEED_LEN, K, rows, hp, n_mask=nm, snapshot_every=every)
        np.testing.assert_array_equal(ids, ids0)
        np.testing.assert_array_equal(cos, cos0)
        # an n_mask = 0 step behind an n_mask = 1 step that kept ANOTHER row of some sequence is refused, per row
        bad = np.array([[0, 0, 0], [0, 1, 0]], dtype=np.int32)
        with pytest.raises(native.NativeError, match="n_mask=0 re-use") as ei:
            su.engine.generate_rows(init, L, SEED_LEN, K, bad, hp, n_mask=[1, 0], snapshot_every=2)
        assert ei.value.code == native.ERR_STATE
    finally:
        su.engine.close()


@pytest.mark.parametrize("prec", [BF16, SPLIT, REFINE])
def test_different_orders_per_row_equal_one_call_per_order(prec):
    R, L, K, I = 8, 6, 64, 2
    su, emb = _random_setup(prec, R)
    try:
        eng = su.engine
        eng.set_image_embeds(emb)
        init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)
        hp = Engine.hyper(0.02, 2.0, 0.1)
        orders = _shuffles(R, L, 11)
        cols, ref_ids, ref_cos = [], [], []
        if prec == REFINE:
            eng.refine_guard(reset=True)
        for j, o in enumerate(orders):
            pos, nm, every = harness.order_positions("shuffle", L, I, order_list=o)
            cols.append(pos)
            i_, c_ = eng.generate(R, init, L, SEED_LEN, K, pos, hp, n_mask=nm, snapshot_every=every)
            ref_ids.append(i_[:, j])
            ref_cos.append(c_[:, j])
        if prec == REFINE:
            assert eng.refine_guard(reset=True)["tripped"] == 0
        ids, cos = eng.generate_rows(init, L, SEED_LEN, K, np.array(cols, dtype=np.int32).T, hp, n_mask=nm, snapshot_every=every)
        np.testing.assert_array_equal(ids, np.stack(ref_ids, axis=1))
        if prec == REFINE:
            assert eng.refine_guard(reset=True)["tripped"] == 0
        else:
            _cos_equal(prec, cos, np.stack(ref_cos, axis=1))
        # the same rows split over two streams (4 + 4)
        grp = EngineGroup(eng, streams=2, min_images=2)
        grp.set_image_embeds(emb)
        ids2, cos2 = grp.generate_rows(init, L, SEED_LEN, K, np.array(cols, dtype=np.int32).T, hp, n_mask=nm, snapshot_every=every)
        grp.close(parent=False)
        np.testing.assert_array_equal(ids2, ids)
    finally:
        su.engine.close()


@pytest.mark.parametrize("prec", [BF16, F32, SPLIT])
def test_several_rows_of_one_image(prec):
    """One resident image, six rows, six orders.  Reference arm at the same row count: the embedding handed over six times,
    one czc_generate call per order, row j of call j."""
    R, L, K, I = 6, 6, 64, 2
    su, emb = _random_setup(prec, 2)
    try:
        eng = su.engine
        init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)
        hp = Engine.hyper(0.02, 2.0, 0.1)
        orders = _shuffles(R, L, 21)
        cols, ref_ids, ref_cos = [], [], []
        eng.set_image_embeds(np.repeat(emb[1:2], R, axis=0))
        for j, o in enumerate(orders):
            pos, nm, every = harness.order_positions("shuffle", L, I, order_list=o)
            cols.append(pos)
            i_, c_ = eng.generate(R, init, L, SEED_LEN, K, pos, hp, n_mask=nm, snapshot_every=every)
            ref_ids.append(i_[:, j])
            ref_cos.append(c_[:, j])
        rows = np.array(cols, dtype=np.int32).T
        eng.set_image_embeds(emb[1:2])
        ids, cos = eng.generate_rows(init, L, SEED_LEN, K, rows, hp, image_of_row=[0] * R, n_mask=nm, snapshot_every=every)
        np.testing.assert_array_equal(ids, np.stack(ref_ids, axis=1))
        _cos_equal(prec, cos, np.stack(ref_cos, axis=1))
        # two resident images, every row names the second: an image_of_row that is ignored would polish row 0 for image 0
        eng.set_image_embeds(emb)
        ids, cos = eng.generate_rows(init, L, SEED_LEN, K, rows, hp, image_of_row=[1] * R, n_mask=nm, snapshot_every=every)
        np.testing.assert_array_equal(ids, np.stack(ref_ids, axis=1))
        _cos_equal(prec, cos, np.stack(ref_cos, axis=1))
        # the resident batch is what it was: a plain call on the two images still runs
        eng.generate(2, init, L, SEED_LEN, K, cols[0], hp, n_mask=nm, snapshot_every=every)
    finally:
        su.engine.close()


def test_limits_are_argument_errors():
    meta, arr = load_case("tiny_senti_seq")
    L, K = meta["L"], meta["K"]
    su = _setup(meta, F32)
    try:
        eng = su.engine
        eng.set_image_embeds(arr["image_embeds"])
        hp = _hyper(meta)
        init = su.bert_tok.encode(meta["prompt"] + su.bert_tok.mask_token * L)
        seq = np.repeat(np.arange(L, dtype=np.int32)[:, None], 2, axis=1)
        mixed = seq.copy()
        mixed[:, 1] = mixed[::-1, 1]
        for bad_pos in (np.full((L, 2), L, np.int32), np.full((L, 2), -1, np.int32)):
            with pytest.raises(native.NativeError, match="position out of range") as ei:
                eng.generate_rows(init, L, SEED_LEN, K, bad_pos, hp)
            assert ei.value.code == native.ERR_ARG
        for bad_ior in ([0, 2], [-1, 0]):
            with pytest.raises(native.NativeError, match="image_of_row") as ei:
                eng.generate_rows(init, L, SEED_LEN, K, seq, hp, image_of_row=bad_ior)
            assert ei.value.code == native.ERR_ARG
        with pytest.raises(native.NativeError, match="image_of_row") as ei:   # NULL = identity needs R == resident batch
            eng.generate_rows(init, L, SEED_LEN, K, np.repeat(seq, 2, axis=1), hp)
        assert ei.value.code == native.ERR_ARG

        calls = []

        def scorer(inp, cand, gen_idx):  # a pure function of its rows, as the reference's scorer is
            calls.append((inp.shape[0], gen_idx))
            return ((cand % 7).astype(np.float32) - 3.0) * 0.1

        eng.set_control_callback(scorer)
        with pytest.raises(native.NativeError, match="control callback.*czc_set_lexicon") as ei:
            eng.generate_rows(init, L, SEED_LEN, K, mixed, hp)
        assert ei.value.code == native.ERR_ARG and not calls
        eng.generate_rows(init, L, SEED_LEN, K, mixed, Engine.hyper(meta["alpha"], meta["beta"], meta["temperature"]))
        assert not calls  # an uncontrolled call never reaches the callback, so differing positions are fine
        ids0, cos0 = eng.generate(2, init, L, SEED_LEN, K, list(range(L)), hp)
        n0 = len(calls)
        ids, cos = eng.generate_rows(init, L, SEED_LEN, K, seq, hp)
        assert calls[n0:] == calls[:n0] == [(2, SEED_LEN + p) for p in range(L)]
        np.testing.assert_array_equal(ids, ids0)
        np.testing.assert_array_equal(cos, cos0)
        eng.set_control_callback(None)
        eng.generate_rows(init, L, SEED_LEN, K, mixed, hp)  # the tables serve differing positions
    finally:
        su.engine.close()


def _objects(meta, B):  # as tests/test_dropin_gpu.py builds the synthetic models
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
    return lm, clip, bt, imgs, synth.make_token_mask(sv)


def test_run_generation_samples_equals_the_serial_sample_loop(monkeypatch):
    import utils
    from conzic_amd import runtime
    from gen_utils import generate_caption
    monkeypatch.setenv("CZC_PRECISION", "f32")
    meta, _ = load_case("tiny_shuffle")
    B, S, L = 3, 3, 10   # 45 BERT rows per serial call, 135 in the rows call: both above the skinny kernel's 32
    logger = logging.getLogger("rows-test")
    names = [f"img{j}" for j in range(B)]
    kw = dict(prompt=meta["prompt"], batch_size=B, max_len=L, top_k=meta["K"], temperature=meta["temperature"], max_iter=2,
              alpha=meta["alpha"], beta=meta["beta"], generate_order="shuffle")
    lm, clip, tok, imgs, mask = _objects(meta, B)
    try:
        utils.set_seed(meta["seed"])
        m1 = mask.copy()
        serial = [generate_caption(names, lm, clip, tok, imgs, m1, logger, **kw) for _ in range(S)]
        st_py, st_np = random.getstate(), np.random.get_state()
        utils.set_seed(meta["seed"])
        m2 = mask.copy()
        got = runtime.run_generation_samples("shuffle", S, names, lm, clip, tok, imgs, m2, meta["prompt"], logger, L, meta["K"],
                                             meta["temperature"], meta["alpha"], meta["beta"], 2, B)
        assert random.getstate() == st_py
        assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), st_np))
        np.testing.assert_array_equal(m1, m2)
        assert len(got) == S
        for (t_ref, s_ref), (t, s) in zip(serial, got):
            assert t == t_ref                      # every sweep's captions and the best-caption entry
            assert [len(x) for x in s] == [len(x) for x in s_ref]
            np.testing.assert_allclose(np.array(s), np.array(s_ref), atol=2e-6)
        assert len({tuple(t[-2]) for t, _ in got}) > 1  # the samples took different orders to different captions
    finally:
        runtime.evict()


def test_demo_cli_batch_samples_prints_the_serial_captions(caplog):
    """`demo_cli --synthetic --order shuffle --samples_num 3` with and without --batch_samples: same orders, same captions."""
    from conzic_amd import demo_cli, runtime
    argv = ["--synthetic", "--order", "shuffle", "--samples_num", "3", "--control_scores", "table"]  # tables whatever nltk does
    out = []
    for extra in ([], ["--batch_samples"]):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            demo_cli.main(argv + extra)
        out.append([r.getMessage() for r in caplog.records])
        runtime.evict()
    for kind in ("Order_list", "final caption", "best caption"):
        serial, batched = ([m for m in o if m.startswith(kind)] for o in out)
        assert len(serial) == 3 and batched == serial, kind
    assert not any("one call at a time" in m for m in out[1])  # the batched arm did go through czc_generate_rows


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


@pytest.mark.parametrize("predrawn", [False, True])
def test_exact_control_with_differing_orders_calls_the_engine_once_per_sample(predrawn, standin, monkeypatch, caplog):
    """The host scorer is told one position per step: shuffle samples then run one engine call each -- whether
    run_generation_samples draws the orders or is handed them -- with the serial loop's results, RNG state and a log line."""
    import utils
    from conzic_amd import runtime
    from control_gen_utils import control_generate_caption
    monkeypatch.setenv("CZC_PRECISION", "f32")
    monkeypatch.delenv("CZC_CONTROL", raising=False)   # auto -> exact where nltk imports
    meta, _ = load_case("tiny_senti_ctx")
    B, S, L, K, I = meta["B"], 3, meta["L"], meta["K"], 2
    logger = logging.getLogger("rows-test")
    names = [f"img{j}" for j in range(B)]
    lm, clip, tok, imgs, mask = _objects(meta, B)
    assert clip.lexicon is None and clip.pos_tags is None
    try:
        utils.set_seed(meta["seed"])
        m1 = mask.copy()
        serial = [control_generate_caption(names, lm, clip, tok, imgs, m1, logger, prompt=meta["prompt"], batch_size=B, max_len=L,
                                           top_k=K, temperature=meta["temperature"], max_iter=I, alpha=meta["alpha"],
                                           beta=meta["beta"], gamma=meta["gamma"], ctl_type="sentiment", style_type=meta["style"],
                                           generate_order="shuffle") for _ in range(S)]
        st_py = random.getstate()
        eng = runtime.get_engine(lm, clip, tok)
        calls0 = eng._ctl_scorer.calls
        assert calls0 == S * I * L
        utils.set_seed(meta["seed"])
        sched = harness.sample_schedules("shuffle", L, I, S) if predrawn else None
        assert sched is None or len({tuple(o) for o in sched[3]}) > 1
        m2 = mask.copy()
        with caplog.at_level(logging.INFO, logger="rows-test"):
            got = runtime.run_generation_samples("shuffle", S, names, lm, clip, tok, imgs, m2, meta["prompt"], logger, L, K,
                                                 meta["temperature"], meta["alpha"], meta["beta"], I, B, gamma=meta["gamma"],
                                                 ctl_signal=meta["style"], schedules=sched)
        assert any("one call at a time" in r.getMessage() for r in caplog.records)
        assert random.getstate() == st_py
        assert eng._ctl_scorer.calls - calls0 == S * I * L   # the scorer saw every step of every sample
        np.testing.assert_array_equal(m1, m2)
        assert len(got) == S
        for (t_ref, s_ref), (t, s) in zip(serial, got):
            assert t == t_ref
            np.testing.assert_array_equal(np.array(s), np.array(s_ref))   # the same engine calls: the same bits
    finally:
        runtime.evict()


@pytest.mark.parametrize("control", ["exact", "table"])
def test_run_cli_batch_samples_writes_the_serial_files(control, standin, monkeypatch, tmp_path):
    """run_cli with its defaults (controllable, sentiment, shuffle), 2 batches x 3 samples: --batch_samples writes the files the
    sample loop writes, in the exact control mode (one engine call per sample) and with tables (one rows call per batch)."""
    import json
    import os
    from PIL import Image
    from conzic_amd import run_cli, runtime
    monkeypatch.setenv("CZC_PRECISION", "f32")
    monkeypatch.setenv("CZC_CONTROL", control)
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    for j, u in enumerate(synth.make_images_u8(4, 40)):
        Image.fromarray(u).save(img_dir / f"im{j}.png")
    outs = []
    for extra in ([], ["--batch_samples"]):
        out_dir = tmp_path / ("rows" if extra else "loop")
        out_dir.mkdir()
        monkeypatch.chdir(out_dir)
        run_cli.main(["--synthetic", "--tiny", "--caption_img_path", str(img_dir), "--batch_size", "2", "--samples_num", "3",
                      "--sentence_len", "5", "--candidate_k", "12", "--num_iterations", "2"] + extra)
        runtime.evict()
        files = {}
        for root, _, fs in os.walk(out_dir / "results"):
            for f in fs:
                files[os.path.relpath(os.path.join(root, f), out_dir)] = json.load(open(os.path.join(root, f)))
        outs.append(files)
    assert len(outs[0]) == 3 * 3 and set(outs[0]) == set(outs[1])
    for k in outs[0]:
        assert len(outs[0][k]) == 4 and outs[1][k] == outs[0][k], k


def test_group_generate_rows_after_encode_images():
    """EngineGroup.generate_rows on embeds the group encoded itself: encode_images returns the un-normalised embeds that
    set_image_embeds takes, so re-dealing them by row gives the one-engine result."""
    import torch
    B, L, K = 4, 5, 12
    su = harness.build_synthetic(True, F32)
    try:
        eng = su.engine
        pix = synth.pixels_from_u8(synth.make_images_u8(B, su.clip_cfg.v_image))
        init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)
        hp = Engine.hyper(0.02, 2.0, 0.1)
        orders = _shuffles(6, L, 5)
        rows = np.array([harness.order_positions("shuffle", L, 2, order_list=o)[0] for o in orders], dtype=np.int32).T
        ior = [0, 1, 2, 3, 3, 0]
        emb = eng.encode_images(pix)
        ids0, cos0 = eng.generate_rows(init, L, SEED_LEN, K, rows, hp, image_of_row=ior)
        eng.set_image_embeds(emb)   # what encode_images returned is what set_image_embeds takes
        ids1, cos1 = eng.generate_rows(init, L, SEED_LEN, K, rows, hp, image_of_row=ior)
        np.testing.assert_array_equal(ids1, ids0)
        np.testing.assert_array_equal(cos1, cos0)
        grp = EngineGroup(eng, streams=2, min_images=2)
        np.testing.assert_array_equal(grp.encode_images(torch.from_numpy(pix).to("cuda:0")), emb)
        ids2, cos2 = grp.generate_rows(init, L, SEED_LEN, K, rows, hp, image_of_row=ior)
        grp.close(parent=False)
        np.testing.assert_array_equal(ids2, ids0)
        np.testing.assert_allclose(cos2, cos0, atol=2e-6)
    finally:
        su.engine.close()
