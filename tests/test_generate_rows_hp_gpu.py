"""-m gpu: czc_generate_rows_hp (include/conzic_hip.h) -- a czc_hyper per row: temperature, alpha / beta / gamma, control signal
and its sign are the row's own in the four kernels that take hyper-parameters.  The yardstick of a row is the existing scalar call
(czc_generate_rows_len / czc_generate_rows_from) on ALL rows with that row's hyper-parameters -- the same row count, so the
parent's behaviour -- and, for temperature and fusion, the CPU oracle.  Tiny synthetic towers, K = 200, R = 6 rows over two
images, L <= 6, two shuffle sweeps."""
import random

import numpy as np
import pytest
import torch

from conzic_amd import harness, lengths, native, synth
from conzic_amd.engine import Engine

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT, REFINE = native.PREC_F32, native.PREC_BF16, native.PREC_SPLIT, native.PREC_REFINE
IDLE = native.POS_IDLE
K = 200
PROMPT = "Image of a"
SEED_LEN = 4
MIXED = [3, 6, 4, 6, 1, 5]
MIXED_IOR = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
TEMPLATE = ["DET", "ADJ", "NOUN", ""]
SETTINGS = [(0.02, 2.0, 0.1), (0.7, 1.0, 1.0), (0.1, 3.0, 0.3)]   # (alpha, beta, temperature)


def _plain(i):
    a, b, t = SETTINGS[i]
    return Engine.hyper(a, b, t)


CAPTION = lambda: Engine.hyper(0.02, 2.0, 0.1)                                # noqa: E731
POSITIVE = lambda: Engine.hyper(0.1, 2.0, 0.1, 0.5)                           # noqa: E731
NEGATIVE = lambda: Engine.hyper(0.1, 2.0, 0.1, 0.5, negative=True)            # noqa: E731
POS = lambda: Engine.hyper(0.1, 2.0, 0.1, 0.5, control="pos")                 # noqa: E731
# rows [caption, positive, negative, POS, positive, caption]; rows 1 and 2 polish the same image at the same length
SIGNALS = [CAPTION, POSITIVE, NEGATIVE, POS, POSITIVE, CAPTION]
SIG_LENS = [5, 6, 6, 4, 3, 6]
SIG_IOR = np.array([0, 1, 1, 0, 0, 1], dtype=np.int32)


def _tiny(prec, n_img=2):
    su = harness.build_synthetic(True, prec, lexicon=True)
    su.engine.set_pos(synth.make_pos_tags(len(su.sv.bert_tokens)), synth.pos_template_masks(TEMPLATE))
    emb = np.random.default_rng(3).standard_normal((n_img, su.clip_cfg.proj)).astype(np.float32)
    su.engine.set_image_embeds(emb)
    return su, emb


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _key(h):
    return bytes(h)


def _against_scalar_calls(eng, prec, start, lens, pos, n_mask, hps, ior, ids, cos, tag):
    """For each distinct hyper h of `hps`: the scalar call on all rows with h, compared on the rows that carry h.  Ids identical;
    cosine bits identical on F32 / BF16, atol 1e-6 on SPLIT / REFINE (their second tower picks kernels by the launch's row
    count, and the companions of a row in the launch differ between the two calls)."""
    seen = {}
    for r, h in enumerate(hps):
        seen.setdefault(_key(h), (h, []))[1].append(r)
    assert len(seen) > 1
    for h, sel in seen.values():
        ref_ids, ref_cos = eng.generate_rows_len(start, lens, SEED_LEN, K, pos, h, image_of_row=ior, n_mask=n_mask)
        d = float(np.abs(cos[:, sel] - ref_cos[:, sel]).max())
        print(f"[rows_hp] {tag} prec {prec} rows {sel}: max |d cos| {d:.3e}, {int((ids[:, sel] != ref_ids[:, sel]).sum())} ids differ")
        np.testing.assert_array_equal(ids[:, sel], ref_ids[:, sel])
        if prec in (F32, BF16):
            np.testing.assert_array_equal(_bits(cos[:, sel]), _bits(ref_cos[:, sel]))
        else:
            np.testing.assert_allclose(cos[:, sel], ref_cos[:, sel], rtol=0, atol=1e-6)


@pytest.mark.parametrize("memo", [0, 1])
@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_uniform_hypers_are_the_existing_call(prec, memo):
    """R equal entries: ids and cosine bits of czc_generate_rows_len on mixed lengths, and of czc_generate_rows_from with
    lens = None on rows that fill the stride."""
    su, _ = _tiny(prec)
    eng = su.engine
    try:
        eng.set_option("memo_rows", memo)
        hp = POSITIVE()
        start = lengths.length_rows(su.bert_tok, PROMPT, MIXED)
        pos, n_mask, _ = lengths.length_schedules(MIXED, "shuffle", 2, rng=random.Random(1))
        ids0, cos0 = eng.generate_rows_len(start, MIXED, SEED_LEN, K, pos, hp, image_of_row=MIXED_IOR, n_mask=n_mask)
        ids1, cos1 = eng.generate_rows_hp(start, MIXED, SEED_LEN, K, pos, [POSITIVE() for _ in MIXED], image_of_row=MIXED_IOR, n_mask=n_mask)
        np.testing.assert_array_equal(ids0, ids1)
        np.testing.assert_array_equal(_bits(cos0), _bits(cos1))
        L = 6
        full = [L] * 6
        start = lengths.length_rows(su.bert_tok, PROMPT, full)
        pos, _, every = lengths.length_schedules(full, "shuffle", 2, rng=random.Random(2))
        assert every == L and (pos != IDLE).all()
        ids0, cos0 = eng.generate_rows_from(start, L, SEED_LEN, K, pos, hp, image_of_row=MIXED_IOR, snapshot_every=L)
        ids1, cos1 = eng.generate_rows_hp(start, None, SEED_LEN, K, pos, [POSITIVE() for _ in full], image_of_row=MIXED_IOR)
        np.testing.assert_array_equal(ids0, ids1)
        np.testing.assert_array_equal(_bits(cos0), _bits(cos1))
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_mixed_alpha_beta_temperature(prec):
    """Three (alpha, beta, temperature) settings over six rows of mixed lengths, no control: every row returns what the scalar
    call with its setting returns for it."""
    su, _ = _tiny(prec)
    eng = su.engine
    try:
        hps = [_plain(r % 3) for r in range(6)]
        start = lengths.length_rows(su.bert_tok, PROMPT, MIXED)
        pos, n_mask, _ = lengths.length_schedules(MIXED, "shuffle", 2, rng=random.Random(2))
        ids, cos = eng.generate_rows_hp(start, MIXED, SEED_LEN, K, pos, hps, image_of_row=MIXED_IOR, n_mask=n_mask)
        _against_scalar_calls(eng, prec, start, MIXED, pos, n_mask, hps, MIXED_IOR, ids, cos, "mixed a/b/T")
    finally:
        eng.close()


def _signal_batch(su, sweeps, seed):
    start = lengths.length_rows(su.bert_tok, PROMPT, SIG_LENS)
    pos, n_mask, every = lengths.length_schedules(SIG_LENS, "shuffle", sweeps, rng=random.Random(seed))
    pos = pos.copy()
    pos[:, 2] = pos[:, 1]   # the positive and the negative row of image 1 share one order: only `negative` tells them apart
    return start, np.ascontiguousarray(pos), n_mask, every


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_mixed_control_signals(prec):
    """Rows [caption, positive, negative, POS, positive, caption] over two images with their own shuffle orders, served by the
    control tables: every row returns what the scalar call under its signal returns for it, and the positive and the negative
    row of one image (same length, same order) differ."""
    su, _ = _tiny(prec)
    eng = su.engine
    try:
        hps = [f() for f in SIGNALS]
        start, pos, n_mask, _ = _signal_batch(su, 2, 4)
        ids, cos = eng.generate_rows_hp(start, SIG_LENS, SEED_LEN, K, pos, hps, image_of_row=SIG_IOR, n_mask=n_mask)
        _against_scalar_calls(eng, prec, start, SIG_LENS, pos, n_mask, hps, SIG_IOR, ids, cos, "signals")
        assert (ids[:, 1] != ids[:, 2]).any()
    finally:
        eng.close()


def test_per_row_settings_against_the_cpu_oracle():
    """F32, three rows of lengths [2, 5, 7], no control, one sequential sweep, row r under SETTINGS[r]: every row against a chain
    of oracle.step.polish_step with the row's temperature, alpha and beta.  Ids equal, winner cosines within 2e-5 (the bound of
    the trajectory goldens).  Pins the per-row temperature and fusion to something that is not this engine."""
    from oracle import models as M, step as S, text as T
    lens = [2, 5, 7]
    su, _ = _tiny(F32, 3)
    eng = su.engine
    try:
        sv = su.sv
        o = S.Oracle(M.to_torch(synth.make_bert_weights(su.bert_cfg, 11)), su.bert_cfg,
                     M.to_torch(synth.make_clip_weights(su.clip_cfg, 12)), su.clip_cfg, sv.bert_tokens,
                     T.ClipBpe(sv.clip_vocab, sv.clip_merges))
        emb = np.random.default_rng(0).standard_normal((3, su.clip_cfg.proj)).astype(np.float32)
        eng.set_image_embeds(emb)
        start = lengths.length_rows(su.bert_tok, PROMPT, lens)
        pos, n_mask, _ = lengths.length_schedules(lens, "sequential", 1)
        ids, cos = eng.generate_rows_hp(start, lens, SEED_LEN, K, pos, [_plain(r) for r in range(3)], n_mask=n_mask)
        for r, n in enumerate(lens):
            alpha, beta, temp = SETTINGS[r]
            inp = torch.tensor(o.init_text(PROMPT, n, 1))
            tmask = torch.from_numpy(su.token_mask.copy())
            cur = None
            for p in range(n):
                o.update_token_mask(tmask, n, p)
                inp[:, SEED_LEN + p] = o.mask_id
                res = S.polish_step(o, inp, torch.from_numpy(emb[r:r + 1]), tmask, SEED_LEN + p, K, temp, alpha, beta)
                cur = float(res["cur_clip"][0])
            print(f"[rows_hp] oracle row {r} (L = {n}, {SETTINGS[r]}): |d cos| {abs(float(cos[0, r]) - cur):.3e}")
            np.testing.assert_array_equal(ids[0, r, :SEED_LEN + n + 1], inp[0].numpy())
            assert abs(float(cos[0, r]) - cur) <= 2e-5
    finally:
        eng.close()


def test_idle_steps_memo_rows_and_compact_batches():
    """harness.converging_setup (the tiny random towers keep moving), the mixed-control batch over two images, eight shuffle
    sweeps in which the shorter rows idle at the end of every sweep, every step snapshotted: option "memo_rows" on returns the
    ids of the option off, with hits -- the steps behind a hit ran on compact batches, which carried each running row's own
    record."""
    su, _, _, _, seed_len = harness.converging_setup(B=2, L=6)
    assert seed_len == SEED_LEN
    eng = su.engine
    try:
        V = len(su.sv.bert_tokens)
        eng.set_lexicon(synth.make_lexicon(V))
        eng.set_pos(synth.make_pos_tags(V), synth.pos_template_masks(TEMPLATE))
        hps = [f() for f in SIGNALS]
        start, pos, n_mask, _ = _signal_batch(su, 8, 12)
        assert (pos == IDLE).any()
        ran = int((pos != IDLE).sum())
        out = {}
        for on in (0, 1):
            eng.set_option("memo_rows", on)
            eng.profile_reset()
            ids, _ = eng.generate_rows_hp(start, SIG_LENS, SEED_LEN, K, pos, hps, image_of_row=SIG_IOR, n_mask=n_mask, snapshot_every=1)
            out[on] = (ids, eng.memo_rows_stats(), eng.stats())
        print(f"[rows_hp] memo_rows {out[1][1]} of {ran} row-steps; clip_seqs {out[0][2]['clip_seqs']} -> {out[1][2]['clip_seqs']}")
        np.testing.assert_array_equal(out[0][0], out[1][0])
        assert out[0][1] == dict(hit_row_steps=0, row_steps=0)
        assert out[1][1]["row_steps"] == ran and out[1][1]["hit_row_steps"] > 0
        assert out[0][2]["clip_seqs"] == K * ran   # idle rows are compacted away with the option off as well
    finally:
        eng.close()


def test_refine_engine_with_a_beta_per_row():
    """CZC_PREC_REFINE, beta in {1, 2, 4} over six rows: the mass threshold and the margin gate's beta are per row.  Ids equal the
    scalar calls', the second pass and the gate ran, and the guard is not tripped."""
    su, _ = _tiny(REFINE)
    eng = su.engine
    try:
        hps = [Engine.hyper(0.02, (1.0, 2.0, 4.0)[r % 3], 0.1) for r in range(6)]
        start = lengths.length_rows(su.bert_tok, PROMPT, MIXED)
        pos, n_mask, _ = lengths.length_schedules(MIXED, "shuffle", 2, rng=random.Random(6))
        eng.refine_guard(reset=True)
        eng.profile_reset()
        ids, cos = eng.generate_rows_hp(start, MIXED, SEED_LEN, K, pos, hps, image_of_row=MIXED_IOR, n_mask=n_mask)
        st, guard = eng.stats(), eng.refine_guard(reset=True)
        print(f"[rows_hp] refine: {st['refine_seqs']} re-encoded, {st['gated_image_steps']} of {st['gate_image_steps']} gated, guard {guard}")
        assert st["refine_seqs"] > 0 and st["refine_rows"] > 0 and st["gate_image_steps"] > 0
        assert guard["tripped"] == 0
        _against_scalar_calls(eng, REFINE, start, MIXED, pos, n_mask, hps, MIXED_IOR, ids, cos, "refine beta")
    finally:
        eng.close()


def test_argument_errors_leave_the_engine_usable():
    su = harness.build_synthetic(True, F32, lexicon=True)   # no czc_set_pos
    eng = su.engine
    try:
        eng.set_image_embeds(np.random.default_rng(3).standard_normal((2, su.clip_cfg.proj)).astype(np.float32))
        start = lengths.length_rows(su.bert_tok, PROMPT, MIXED)
        pos, n_mask, _ = lengths.length_schedules(MIXED, "sequential", 1)
        good = [_plain(r % 3) for r in range(6)]
        want, _ = eng.generate_rows_hp(start, MIXED, SEED_LEN, K, pos, good, image_of_row=MIXED_IOR, n_mask=n_mask)
        eng.profile_reset()

        def refused(code, match, hps, p=pos):
            with pytest.raises(native.NativeError, match=match) as ei:
                eng.generate_rows_hp(start, MIXED, SEED_LEN, K, p, hps, image_of_row=MIXED_IOR, n_mask=n_mask)
            assert ei.value.code == code
            assert eng.stats()["steps"] == 0   # refused before any GPU work
            ids, _ = eng.generate_rows_hp(start, MIXED, SEED_LEN, K, pos, good, image_of_row=MIXED_IOR, n_mask=n_mask)
            np.testing.assert_array_equal(ids, want)
            eng.profile_reset()

        def with_row(r, **kw):
            hps = [_plain(i % 3) for i in range(6)]
            for k, v in kw.items():
                setattr(hps[r], k, v)
            return hps

        refused(native.ERR_ARG, "control outside", with_row(4, control=3))
        refused(native.ERR_ARG, "temperature", with_row(5, temperature=0.0))
        refused(native.ERR_ARG, "temperature", with_row(0, temperature=float("inf")))
        refused(native.ERR_ARG, "must be finite", with_row(2, alpha=float("nan")))
        refused(native.ERR_STATE, "POS path needs czc_set_pos", with_row(3, control=2, gamma=0.5))
        bad = pos.copy()
        bad[0, 0] = 3                                           # everything czc_generate_rows_len checks: row 0 has L = 3
        refused(native.ERR_ARG, "position outside", good, p=bad)
        with pytest.raises(ValueError):
            eng.generate_rows_hp(start, MIXED, SEED_LEN, K, pos, good[:5], image_of_row=MIXED_IOR, n_mask=n_mask)
        # a host scorer is configured for one signal: rows of differing control are refused, differing alpha / beta are not
        lex = synth.make_lexicon(len(su.sv.bert_tokens))
        eng.set_control_callback(lambda inp, cand, gen_idx: lex[cand].astype(np.float32))
        try:
            refused(native.ERR_ARG, "control callback", with_row(1, control=1, gamma=0.5))
            L = 6
            full = [L] * 6
            rows = lengths.length_rows(su.bert_tok, PROMPT, full)
            same = np.ascontiguousarray(np.repeat(np.arange(L, dtype=np.int32)[:, None], 6, axis=1))
            hps = [Engine.hyper(*SETTINGS[r % 3][:2], SETTINGS[r % 3][2], 0.5) for r in range(6)]
            eng.generate_rows_hp(rows, full, SEED_LEN, K, same, hps, image_of_row=MIXED_IOR)
        finally:
            eng.set_control_callback(None)
    finally:
        eng.close()
