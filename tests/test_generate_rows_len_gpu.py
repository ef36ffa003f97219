"""-m gpu: czc_generate_rows_len (include/conzic_hip.h) -- a sentence length per row: BERT on packed ragged rows, each row at its
own position embeddings and attention span, the padding tail never read.  Held against czc_generate_rows_from at each row's own
length (bit for bit where the call is the same call, ids + 1e-6 where only the BERT row count differs) and, for the ragged
embeddings and attention themselves, against the CPU oracle."""
import random

import numpy as np
import pytest
import torch

from conzic_amd import harness, lengths, native, synth
from conzic_amd.engine import Engine, EngineGroup

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT, REFINE = native.PREC_F32, native.PREC_BF16, native.PREC_SPLIT, native.PREC_REFINE
IDLE = native.POS_IDLE
K = 200
PROMPT = "Image of a"
SEED_LEN = 4
MIXED = [3, 6, 4, 6, 1, 5]
MIXED_IOR = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)


def _tiny(prec, n_img):
    su = harness.build_synthetic(True, prec)
    emb = np.random.default_rng(3).standard_normal((n_img, su.clip_cfg.proj)).astype(np.float32)
    su.engine.set_image_embeds(emb)
    return su, emb, Engine.hyper(0.02, 2.0, 0.1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _per_length(eng, start, lens, pos, hp, ior, sweeps):
    """The reference: one czc_generate_rows_from call per distinct length, on that length's rows cut to their own T_r, with their
    columns of the schedule (a row's visits sit in the first L_r steps of every sweep).  Returns (ids [sweeps, R, T] with 0 behind
    every row's own tokens, cos [sweeps, R])."""
    R, T = start.shape
    every = pos.shape[0] // sweeps
    ids, cos = np.zeros((sweeps, R, T), np.int32), np.zeros((sweeps, R), np.float32)
    for Ld in sorted(set(lens)):
        sel = [r for r in range(R) if lens[r] == Ld]
        Td = SEED_LEN + Ld + 1
        p = np.ascontiguousarray(pos.reshape(sweeps, every, R)[:, :Ld][:, :, sel].reshape(sweeps * Ld, len(sel)))
        assert (p != IDLE).all()
        i, c = eng.generate_rows_from(np.ascontiguousarray(start[sel, :Td]), Ld, SEED_LEN, K, p, hp, image_of_row=ior[sel], snapshot_every=Ld)
        ids[:, sel, :Td], cos[:, sel] = i, c
    return ids, cos


def _check_tails(ids, lens):
    for r, n in enumerate(lens):
        assert (ids[:, r, SEED_LEN + n + 1:] == 0).all()


@pytest.mark.parametrize("memo", [0, 1])
@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_uniform_lengths_are_generate_rows_from(prec, memo):
    """R = 5 rows of L = 6 that fill the stride, two shuffle sweeps, option "memo_rows" off and on: the ids and the cosine bits of
    czc_generate_rows_from."""
    R, L = 5, 6
    su, _, hp = _tiny(prec, 2)
    eng = su.engine
    try:
        lens = [L] * R
        start = lengths.length_rows(su.bert_tok, PROMPT, lens)
        pos, _, every = lengths.length_schedules(lens, "shuffle", 2, rng=random.Random(1))
        assert every == L and (pos != IDLE).all()
        ior = np.array([0, 1, 0, 1, 1], dtype=np.int32)
        eng.set_option("memo_rows", memo)
        ids0, cos0 = eng.generate_rows_from(start, L, SEED_LEN, K, pos, hp, image_of_row=ior, snapshot_every=L)
        ids1, cos1 = eng.generate_rows_len(start, lens, SEED_LEN, K, pos, hp, image_of_row=ior, snapshot_every=L)
        np.testing.assert_array_equal(ids0, ids1)
        np.testing.assert_array_equal(_bits(cos0), _bits(cos1))
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT])
def test_mixed_lengths_against_per_length_calls(prec):
    """R = 6 rows over two images with lengths [3, 6, 4, 6, 1, 5] (the L = 1 row's only position carries the '.' rule), two
    shuffle sweeps, against one czc_generate_rows_from call per distinct length at that T_r: ids identical, cosines within
    atol = 1e-6 (the bound test_generate_rows_from_gpu.py and test_memo_rows_gpu.py use where only the BERT row count differs);
    the padding tails of the out rows are 0 and bert_rows counts the sum of T_r over the row-steps that ran, not R x T."""
    su, emb, hp = _tiny(prec, 2)
    eng = su.engine
    try:
        sweeps = 2
        start = lengths.length_rows(su.bert_tok, PROMPT, MIXED)
        pos, n_mask, every = lengths.length_schedules(MIXED, "shuffle", sweeps, rng=random.Random(2))
        assert start.shape == (6, SEED_LEN + 6 + 1) and every == 6
        eng.profile_reset()
        ids, cos = eng.generate_rows_len(start, MIXED, SEED_LEN, K, pos, hp, image_of_row=MIXED_IOR, n_mask=n_mask)
        st = eng.stats()
        ref_ids, ref_cos = _per_length(eng, start, MIXED, pos, hp, MIXED_IOR, sweeps)
        print(f"[rows_len] prec {prec}: max |d cos| vs the per-length calls {np.abs(cos - ref_cos).max():.3e}, "
              f"{int((ids != ref_ids).sum())} ids differ")
        np.testing.assert_array_equal(ids, ref_ids)
        np.testing.assert_allclose(cos, ref_cos, rtol=0, atol=1e-6)
        _check_tails(ids, MIXED)
        assert st["bert_rows"] == sweeps * sum(n * (SEED_LEN + n + 1) for n in MIXED)
        assert st["clip_seqs"] == K * sweeps * sum(MIXED)
    finally:
        eng.close()


def test_mixed_lengths_against_the_cpu_oracle():
    """Lengths [2, 5, 7], one sequential sweep, F32: every row against a chain of oracle.step.polish_step at the row's own T_r
    (the oracle test_step_gpu.py::test_minimal_shapes_k1_l1 builds): ids equal, winner cosines within atol = 2e-5 (the bound of
    the trajectory goldens).  Pins the ragged position embeddings and attention to something that is not this engine."""
    from oracle import models as M, step as S, text as T
    lens = [2, 5, 7]
    su, _, hp = _tiny(F32, 3)
    eng = su.engine
    try:
        sv = su.sv
        o = S.Oracle(M.to_torch(synth.make_bert_weights(su.bert_cfg, 11)), su.bert_cfg,
                     M.to_torch(synth.make_clip_weights(su.clip_cfg, 12)), su.clip_cfg, sv.bert_tokens,
                     T.ClipBpe(sv.clip_vocab, sv.clip_merges))
        emb = np.random.default_rng(0).standard_normal((3, su.clip_cfg.proj)).astype(np.float32)
        eng.set_image_embeds(emb)
        start = lengths.length_rows(su.bert_tok, PROMPT, lens)
        pos, n_mask, every = lengths.length_schedules(lens, "sequential", 1)
        ids, cos = eng.generate_rows_len(start, lens, SEED_LEN, K, pos, hp, n_mask=n_mask)
        assert ids.shape == (1, 3, SEED_LEN + 7 + 1)
        _check_tails(ids, lens)
        for r, n in enumerate(lens):
            inp = torch.tensor(o.init_text(PROMPT, n, 1))
            assert inp[0].tolist() == start[r, :SEED_LEN + n + 1].tolist()
            tmask = torch.from_numpy(su.token_mask.copy())
            cur = None
            for p in range(n):
                o.update_token_mask(tmask, n, p)
                inp[:, SEED_LEN + p] = o.mask_id
                res = S.polish_step(o, inp, torch.from_numpy(emb[r:r + 1]), tmask, SEED_LEN + p, K, 0.1, 0.02, 2.0)
                cur = float(res["cur_clip"][0])
            print(f"[rows_len] oracle row {r} (L = {n}): |d cos| {abs(float(cos[0, r]) - cur):.3e}")
            np.testing.assert_array_equal(ids[0, r, :SEED_LEN + n + 1], inp[0].numpy())
            assert abs(float(cos[0, r]) - cur) <= 2e-5
    finally:
        eng.close()


def test_sentiment_tables_on_mixed_lengths():
    """control = 1 with the lexicon table, gamma 0.5, BF16, mixed lengths against the per-length calls: ids identical, cosines
    1e-6.  K = 200 on the tiny vocabulary puts masked ([PAD]) candidates into every step, so a repeat count that read the
    padding tail would change the fused score."""
    su, emb, _ = _tiny(BF16, 2)
    eng = su.engine
    try:
        eng.set_lexicon(synth.make_lexicon(len(su.sv.bert_tokens)))
        hp = Engine.hyper(0.1, 2.0, 0.1, 0.5)
        sweeps = 2
        start = lengths.length_rows(su.bert_tok, PROMPT, MIXED)
        pos, n_mask, _ = lengths.length_schedules(MIXED, "shuffle", sweeps, rng=random.Random(5))
        ids, cos = eng.generate_rows_len(start, MIXED, SEED_LEN, K, pos, hp, image_of_row=MIXED_IOR, n_mask=n_mask)
        ref_ids, ref_cos = _per_length(eng, start, MIXED, pos, hp, MIXED_IOR, sweeps)
        print(f"[rows_len] sentiment: max |d cos| {np.abs(cos - ref_cos).max():.3e}, {int((ids != ref_ids).sum())} ids differ")
        np.testing.assert_array_equal(ids, ref_ids)
        np.testing.assert_allclose(cos, ref_cos, rtol=0, atol=1e-6)
        _check_tails(ids, MIXED)
    finally:
        eng.close()


def _pair_len(eng, start, lens, pos, hp, ior, every, want_cos=True):
    out = {}
    for on in (0, 1):
        eng.set_option("memo_rows", on)
        eng.profile_reset()
        ids, cos = eng.generate_rows_len(start, lens, SEED_LEN, K, pos, hp, image_of_row=ior, snapshot_every=every, want_cos=want_cos)
        out[on] = (ids, cos, eng.stats(), eng.memo_rows_stats())
    eng.set_option("memo_rows", 0)
    return out


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_memo_rows_with_idle_steps_and_lengths_is_exact(prec):
    """harness.converging_setup, 4 images x 4 rows of lengths 6 / 4 / 5 / 3, eight shuffle sweeps (the shorter rows idle at the
    end of every sweep), every step snapshotted: option "memo_rows" off against on gives identical ids and cosine bits
    (CZC_PREC_REFINE as test_memo_rows_is_exact_on_a_converging_batch compares it: ids without cosines, then a per-sweep call
    within 1e-6), with hits and with steps that ran on a compact batch of the rows that missed."""
    B, S, sweeps = 4, 4, 8
    su, _, hp, _, seed_len = harness.converging_setup(B=B, L=6, precision=prec)
    assert seed_len == SEED_LEN
    eng = su.engine
    try:
        lens = [n for n in (6, 4, 5, 3) for _ in range(B)]
        ior = np.tile(np.arange(B, dtype=np.int32), S)
        start = lengths.length_rows(su.bert_tok, PROMPT, lens)
        pos, _, every = lengths.length_schedules(lens, "shuffle", sweeps, rng=random.Random(12))
        ran = int((pos != IDLE).sum())
        t_of = np.array([SEED_LEN + n + 1 for n in lens])
        out = _pair_len(eng, start, lens, pos, hp, ior, 1, want_cos=prec != REFINE)
        np.testing.assert_array_equal(out[0][0], out[1][0])
        if prec != REFINE:
            np.testing.assert_array_equal(_bits(out[0][1]), _bits(out[1][1]))
        _check_tails(out[1][0], lens)
        print(f"[rows_len] prec {prec}: memo_rows {out[1][3]} of {ran} row-steps, bert_rows {out[0][2]['bert_rows']} -> {out[1][2]['bert_rows']}")
        assert out[0][3] == dict(hit_row_steps=0, row_steps=0)
        hits = out[1][3]["hit_row_steps"]
        assert out[1][3]["row_steps"] == ran and 0 < hits < ran
        assert out[0][2]["bert_rows"] == int(((pos != IDLE) * t_of[None, :]).sum())
        assert out[0][2]["clip_seqs"] == K * ran and out[1][2]["clip_seqs"] == K * (ran - hits)
        if prec != SPLIT:   # (the split engine runs a checked step whole unless every row hits)
            # a step that ran with some of its rows hit ran on a compact batch: fewer BERT rows than its running rows hold
            assert out[1][2]["bert_rows"] < out[0][2]["bert_rows"]
            assert out[1][2]["steps"] * len(lens) > ran - hits   # some executed step ran on fewer rows than the batch holds
        if prec == REFINE:
            o2 = _pair_len(eng, start, lens, pos, hp, ior, every)
            np.testing.assert_array_equal(o2[0][0], o2[1][0])
            np.testing.assert_allclose(o2[0][1], o2[1][1], rtol=0, atol=1e-6)
            assert o2[1][3]["hit_row_steps"] > 0
    finally:
        eng.close()


def test_argument_checks_leave_the_engine_usable():
    lens = [2, 4, 3]
    su, emb, hp = _tiny(F32, 3)
    eng = su.engine
    try:
        start = lengths.length_rows(su.bert_tok, PROMPT, lens)
        good, _, every = lengths.length_schedules(lens, "sequential", 1)
        want, _ = eng.generate_rows_len(start, lens, SEED_LEN, K, good, hp)

        def refused(match, rows=start, ln=lens, pos=good, n_mask=None):
            with pytest.raises(native.NativeError, match=match) as ei:
                eng.generate_rows_len(rows, ln, SEED_LEN, K, pos, hp, n_mask=n_mask, snapshot_every=every)
            assert ei.value.code == native.ERR_ARG
            ids, _ = eng.generate_rows_len(start, lens, SEED_LEN, K, good, hp)   # the engine is still usable
            np.testing.assert_array_equal(ids, want)

        refused("len_of_row outside", ln=[0, 4, 3])
        refused("len_of_row outside", ln=[2, 5, 3])          # T - seed_len - 1 = 4
        bad = good.copy()
        bad[2, 0] = 2                                         # row 0 has positions 0 and 1
        refused("position outside", pos=bad)
        bad = good.copy()
        bad[0, 1] = -2
        refused("position outside", pos=bad)
        rows = start.copy()
        rows[0, SEED_LEN + 2 + 1] = 7                         # first column of row 0's tail
        refused(r"must hold id 0", rows=rows)
        rows = start.copy()
        rows[2, -1] = 7                                       # last column of row 2's tail
        refused(r"must hold id 0", rows=rows)
        nm = [2, 0, 1, 1]
        over = np.array([[1, 0, 0], [0, 1, 1], [IDLE, 2, 2], [IDLE, 3, IDLE]], dtype=np.int32)   # row 0: n_mask = 2 at its last position
        refused("masks past the row's last position", pos=over, n_mask=nm)
        rows = start.copy()
        rows[1, 2] = su.bert_cfg.vocab                        # everything czc_generate_rows_from checks
        refused("outside the BERT vocabulary", rows=rows)
        half = np.array([[0, 0, 0], [IDLE, 1, 1], [IDLE, 2, 2], [IDLE, 3, IDLE]], dtype=np.int32)
        refused("whole step group", pos=half, n_mask=nm)
        with pytest.raises(ValueError):
            eng.generate_rows_len(start, lens[:2], SEED_LEN, K, good, hp)
    finally:
        eng.close()


def test_a_host_scorer_needs_one_position_and_one_length():
    """A controlled call with a callback is accepted only when the running rows of every step share position and length; the
    callback then sees T = T_r (the rows without their padding), and the result is the per-length calls' with the same scorer."""
    su, emb, _ = _tiny(F32, 2)
    eng = su.engine
    try:
        lex = synth.make_lexicon(len(su.sv.bert_tokens))
        eng.set_lexicon(lex)
        hp = Engine.hyper(0.1, 2.0, 0.1, 0.5)
        lens = [3, 5, 3, 5]
        ior = np.array([0, 1, 1, 0], dtype=np.int32)
        start = lengths.length_rows(su.bert_tok, PROMPT, lens)
        # the L = 3 rows run steps 0 .. 2 of a sweep, the L = 5 rows steps 3 .. 7, each group in one shared sequential order
        sweep = np.full((8, 4), IDLE, dtype=np.int32)
        sweep[0:3, [0, 2]] = np.arange(3)[:, None]
        sweep[3:8, [1, 3]] = np.arange(5)[:, None]
        pos = np.ascontiguousarray(np.tile(sweep, (2, 1)))
        seen = []

        def scorer(inp, cand, gen_idx):
            seen.append((inp.shape, gen_idx))
            ctx = lex[inp].mean(axis=1, keepdims=True)
            return (lex[cand] + 0.25 * ctx).astype(np.float32)

        eng.set_control_callback(scorer)
        ids, cos = eng.generate_rows_len(start, lens, SEED_LEN, K, pos, hp, image_of_row=ior, snapshot_every=8)
        assert [s for s, _ in seen] == ([(2, SEED_LEN + 3 + 1)] * 3 + [(2, SEED_LEN + 5 + 1)] * 5) * 2
        assert [g for _, g in seen] == ([SEED_LEN + p for p in range(3)] + [SEED_LEN + p for p in range(5)]) * 2
        _check_tails(ids, lens)
        for Ld, sel in ((3, [0, 2]), (5, [1, 3])):
            Td = SEED_LEN + Ld + 1
            p = np.repeat(np.tile(np.arange(Ld, dtype=np.int32), 2)[:, None], 2, axis=1)
            ri, rc = eng.generate_rows_from(np.ascontiguousarray(start[sel, :Td]), Ld, SEED_LEN, K, p, hp, image_of_row=ior[sel],
                                            snapshot_every=Ld)
            np.testing.assert_array_equal(ids[:, sel, :Td], ri)
            np.testing.assert_allclose(cos[:, sel], rc, rtol=0, atol=1e-6)
        # one position, two lengths at a step: refused; so are two positions
        both = np.ascontiguousarray(np.repeat(np.arange(3, dtype=np.int32)[:, None], 4, axis=1))
        with pytest.raises(native.NativeError, match="share one length") as ei:
            eng.generate_rows_len(start, lens, SEED_LEN, K, both, hp, image_of_row=ior, snapshot_every=3)
        assert ei.value.code == native.ERR_ARG
        two = sweep.copy()
        two[0, 2] = 1
        two[1, 2] = 0
        with pytest.raises(native.NativeError, match="control callback") as ei:
            eng.generate_rows_len(start, lens, SEED_LEN, K, two, hp, image_of_row=ior, snapshot_every=8)
        assert ei.value.code == native.ERR_ARG
        eng.set_control_callback(None)
        eng.generate_rows_len(start, lens, SEED_LEN, K, both, hp, image_of_row=ior, snapshot_every=3)   # the tables take both
    finally:
        eng.set_control_callback(None)
        eng.close()


def test_two_streams_return_the_single_engine_bits():
    su, emb, hp = _tiny(F32, 2)
    eng = su.engine
    try:
        start = lengths.length_rows(su.bert_tok, PROMPT, MIXED)
        pos, n_mask, every = lengths.length_schedules(MIXED, "shuffle", 2, rng=random.Random(8))
        ids0, cos0 = eng.generate_rows_len(start, MIXED, SEED_LEN, K, pos, hp, image_of_row=MIXED_IOR, n_mask=n_mask)
        grp = EngineGroup(eng, streams=2, min_images=3)
        try:
            grp.set_image_embeds(emb)
            ids1, cos1 = grp.generate_rows_len(start, MIXED, SEED_LEN, K, pos, hp, image_of_row=MIXED_IOR, n_mask=n_mask)
            assert len(grp.parts(6)) == 2
            np.testing.assert_array_equal(ids0, ids1)
            np.testing.assert_array_equal(_bits(cos0), _bits(cos1))
        finally:
            grp.close(parent=False)
    finally:
        eng.close()
