"""-m gpu: czc_generate_rows_from (include/conzic_hip.h) -- a start row per row and steps a row may sit out (CZC_POS_IDLE):
infilling, resume, polishing a draft.  A step's result depends only on the rows it is given, so everything here is held bit for
bit (or to the bound an existing test uses for the same comparison) against APIs that are pinned to the goldens:
czc_generate_rows, czc_generate and chains of czc_step."""
import random

import numpy as np
import pytest

from conzic_amd import harness, infill, native, synth
from conzic_amd.engine import Engine, EngineGroup
from goldutil import load_case

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT, REFINE = native.PREC_F32, native.PREC_BF16, native.PREC_SPLIT, native.PREC_REFINE
IDLE = native.POS_IDLE
K = 200
PROMPT = "Image of a"
SEED_LEN = 4


def _shuffle_rows(R, L, sweeps, seed):
    """positions int32 [L * sweeps, R]: a shuffle order per row."""
    rng = random.Random(seed)
    cols = []
    for _ in range(R):
        o = list(range(L))
        rng.shuffle(o)
        cols.append(harness.order_positions("shuffle", L, sweeps, order_list=o)[0])
    return np.ascontiguousarray(np.array(cols, dtype=np.int32).T)


def _tiny(prec, R_img, L):
    """Tiny synthetic engine with R_img resident images; (setup, embeds, standard init row, hyper)."""
    su = harness.build_synthetic(True, prec)
    emb = np.random.default_rng(3).standard_normal((R_img, su.clip_cfg.proj)).astype(np.float32)
    su.engine.set_image_embeds(emb)
    init = np.array(su.bert_tok.encode(PROMPT + su.bert_tok.mask_token * L), dtype=np.int32)
    return su, emb, init, Engine.hyper(0.02, 2.0, 0.1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _blank_rows(su, words, blank_sets):
    """Start rows: `words` [R, T] (rows that hold words) with every row's own blank positions set to [MASK]."""
    start = words.copy()
    for r, bl in enumerate(blank_sets):
        for p in bl:
            start[r, SEED_LEN + p] = su.bert_tok.mask_token_id
    return start


def _chain(eng, emb_rows, start, pos, n_mask, L, hp, every, k=K):
    """The reference built from czc_step only.  Resident embeds = one per row; for every step group and every distinct position
    tuple among the rows that are not idle, the group's steps run on a copy of the full [R, T] rows and the result is kept for
    the rows that sit at that tuple.  Returns (ids [S, R, T], cos [S, R]) per snapshot; cos = 0 while a row has not run."""
    eng.set_image_embeds(emb_rows)
    pos = np.asarray(pos)
    n_steps, R = pos.shape
    nm = [1] * n_steps if n_mask is None else list(n_mask)
    rows, cos = start.copy(), np.zeros(R, np.float32)
    out_ids, out_cos = [], []
    for s0, g in harness.memo_groups(nm, n_steps):
        after = [rows.copy() for _ in range(g)]
        after_cos = [cos.copy() for _ in range(g)]
        for tup in sorted({tuple(int(x) for x in pos[s0:s0 + g, r]) for r in range(R)}):
            if tup[0] == IDLE:
                continue
            sel = (pos[s0:s0 + g] == np.array(tup)[:, None]).all(axis=0)
            cur = rows.copy()
            for j, p in enumerate(tup):
                res = eng.step(cur, SEED_LEN + p, k, hp, n_mask=nm[s0 + j], dot_allowed=(p == L - 1), want=("best_cos",))
                after[j][sel] = cur[sel]
                after_cos[j][sel] = res["best_cos"][sel]
        for j in range(g):
            if (s0 + j + 1) % every == 0:
                out_ids.append(after[j].copy())
                out_cos.append(after_cos[j].copy())
        rows, cos = after[-1], after_cos[-1]
    return np.stack(out_ids), np.stack(out_cos)


@pytest.mark.parametrize("memo", [0, 1])
@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_same_start_row_and_no_idle_step_is_generate_rows(prec, memo):
    """R = 5 rows over two images, a shuffle order per row, two sweeps: the standard init row tiled R times gives the ids and
    the cosine bits of czc_generate_rows, with option "memo_rows" off and on."""
    R, L = 5, 6
    su, _, init, hp = _tiny(prec, 2, L)
    eng = su.engine
    try:
        pos = _shuffle_rows(R, L, 2, 1)
        ior = np.array([0, 1, 0, 1, 1], dtype=np.int32)
        eng.set_option("memo_rows", memo)
        ids0, cos0 = eng.generate_rows(init, L, SEED_LEN, K, pos, hp, image_of_row=ior, snapshot_every=L)
        ids1, cos1 = eng.generate_rows_from(np.tile(init, (R, 1)), L, SEED_LEN, K, pos, hp, image_of_row=ior, snapshot_every=L)
        np.testing.assert_array_equal(ids0, ids1)
        np.testing.assert_array_equal(_bits(cos0), _bits(cos1))
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT])
def test_resume_is_exact(prec):
    """Five sweeps in one czc_generate_rows call against two sweeps followed by czc_generate_rows_from from their last snapshot
    with the positions of sweeps 3 to 5: snapshots 3 to 5 bit for bit.  (CZC_PREC_REFINE is left out on purpose: its audit steps
    are placed by sweep index within a call.)"""
    R, L = 6, 5
    su, _, init, hp = _tiny(prec, 2, L)
    eng = su.engine
    try:
        pos = _shuffle_rows(R, L, 5, 2)
        ior = np.array([0, 1, 1, 0, 0, 1], dtype=np.int32)
        ids5, cos5 = eng.generate_rows(init, L, SEED_LEN, K, pos, hp, image_of_row=ior, snapshot_every=L)
        ids2, _ = eng.generate_rows(init, L, SEED_LEN, K, pos[:2 * L], hp, image_of_row=ior, snapshot_every=L)
        np.testing.assert_array_equal(ids2, ids5[:2])
        ids3, cos3 = eng.generate_rows_from(ids2[-1], L, SEED_LEN, K, pos[2 * L:], hp, image_of_row=ior, snapshot_every=L)
        np.testing.assert_array_equal(ids3, ids5[2:])
        np.testing.assert_array_equal(_bits(cos3), _bits(cos5[2:]))
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, SPLIT])
def test_resume_continues_the_reference_trajectory(prec):
    """The reference's tiny shuffle trajectory (tests/golden/tiny_shuffle.npz, two sweeps, its own K = 16): sweep 1 by
    czc_generate, sweep 2 by czc_generate_rows_from from that snapshot; ids equal the golden snapshots, cosines within the
    atol = 2e-5 that test_memo_rows_gpu.py::test_mixed_order_goldens_with_the_option_on uses against the same kind of record.
    (That test loads the full-size one-sweep shuffle golden, which has no second sweep to resume into; this is the tiny one.)"""
    m, a = load_case("tiny_shuffle")
    L, Kg, B = m["L"], m["K"], m["B"]
    su = harness.build_synthetic(m["tiny"], prec, m["bseed"], m["cseed"], m["logit_scale"], m["regular_only"])
    eng = su.engine
    try:
        eng.set_image_embeds(a["image_embeds"])
        init = su.bert_tok.encode(m["prompt"] + su.bert_tok.mask_token * L)
        hp = Engine.hyper(m["alpha"], m["beta"], m["temperature"])
        order = m["order_list"]
        ids1, cos1 = eng.generate(B, init, L, SEED_LEN, Kg, order, hp, snapshot_every=L)
        rest = np.repeat(np.array(order * (m["I"] - 1), dtype=np.int32)[:, None], B, axis=1)
        ids2, cos2 = eng.generate_rows_from(ids1[-1], L, SEED_LEN, Kg, rest, hp, snapshot_every=L)
        ids, cos = np.concatenate([ids1, ids2]), np.concatenate([cos1, cos2])
        assert ids.shape == a["snaps"].shape
        np.testing.assert_array_equal(ids, a["snaps"])
        np.testing.assert_allclose(cos, np.array(m["scores"][:-1], dtype=np.float32), atol=2e-5)
    finally:
        eng.close()


def _idle_case(su, emb, init, hp, L):
    """R = 6 rows over two images whose start rows hold words (a previous call's output) with blank sets of sizes 4, 3, 2, 2, 1
    and 0 set to [MASK]; two sweeps over every row's blanks in a shuffled order of its own, padded with idle steps."""
    eng = su.engine
    ior = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
    eng.set_image_embeds(emb)
    words, _ = eng.generate_rows(init, L, SEED_LEN, K, np.repeat(np.arange(L, dtype=np.int32)[:, None], 6, axis=1), hp,
                                 image_of_row=ior, snapshot_every=L)
    blank_sets = [[0, 1, 3, 4], [1, 2, 4], [0, 4], [2, 3], [3], []]
    start = _blank_rows(su, words[-1], blank_sets)
    pos, n_mask, every = infill.infill_schedules(blank_sets, "shuffle", 2, rng=random.Random(7))
    assert pos.shape == (8, 6) and every == 4
    return ior, start, pos, n_mask, every, blank_sets


@pytest.mark.parametrize("prec", [F32, BF16])
def test_idle_steps_against_a_chain_of_steps(prec):
    """Idle steps against czc_step on the full rows: ids identical, cosines within atol = 1e-6 (the bound
    tests/test_memo_rows_gpu.py uses where a compact batch is compared with a full one), the row without blanks keeps its start
    row with cosine exactly 0.  The call's counters count the rows that ran only; a schedule that is idle everywhere runs
    nothing."""
    L = 5
    su, emb, init, hp = _tiny(prec, 2, L)
    eng = su.engine
    try:
        ior, start, pos, n_mask, every, blank_sets = _idle_case(su, emb, init, hp, L)
        T = start.shape[1]
        eng.set_image_embeds(emb)
        eng.profile_reset()
        ids, cos = eng.generate_rows_from(start, L, SEED_LEN, K, pos, hp, image_of_row=ior, n_mask=n_mask, snapshot_every=every)
        st = eng.stats()
        ref_ids, ref_cos = _chain(eng, emb[ior], start, pos, n_mask, L, hp, every)
        print(f"[rows_from] prec {prec}: max |d cos| vs the czc_step chain {np.abs(cos - ref_cos).max():.3e}")
        np.testing.assert_array_equal(ids, ref_ids)
        np.testing.assert_allclose(cos, ref_cos, rtol=0, atol=1e-6)
        for s in range(ids.shape[0]):
            np.testing.assert_array_equal(ids[s, 5], start[5])
            assert _bits(cos[s, 5]) == 0
            for r, bl in enumerate(blank_sets):   # the given words stay
                given = [c for c in range(T) if c - SEED_LEN not in bl]
                np.testing.assert_array_equal(ids[s, r, given], start[r, given])
        # work is spent on the rows that ran only
        ran = int((pos != IDLE).sum())
        assert ran == 2 * sum(len(b) for b in blank_sets)
        assert st["clip_seqs"] == K * ran
        assert st["bert_rows"] == T * ran
        assert st["steps"] == int((pos != IDLE).any(axis=1).sum())
        # idle everywhere: nothing runs, the start rows come back, every cosine is 0
        eng.set_image_embeds(emb)
        eng.profile_reset()
        ids0, cos0 = eng.generate_rows_from(start, L, SEED_LEN, K, np.full((3, 6), IDLE, dtype=np.int32), hp, image_of_row=ior,
                                            snapshot_every=1)
        st0 = eng.stats()
        assert (st0["clip_rows"], st0["clip_seqs"], st0["bert_rows"], st0["steps"]) == (0, 0, 0, 0)
        np.testing.assert_array_equal(ids0, np.broadcast_to(start, ids0.shape))
        assert (_bits(cos0) == 0).all()
    finally:
        eng.close()


def _converging_infill(prec):
    """The converging setup of tests/test_memo_rows_gpu.py::test_memo_rows_is_exact_on_a_converging_batch rebuilt from harness:
    4 images x 4 rows, L = 6, start rows that hold words with unequal blank counts, eight sweeps."""
    B, S, L, sweeps = 4, 4, 6, 8
    R = B * S
    su, _, hp, init, seed_len = harness.converging_setup(B=B, L=L, precision=prec)
    assert seed_len == SEED_LEN
    eng = su.engine
    ior = np.tile(np.arange(B, dtype=np.int32), S)
    eng.set_option("memo_rows", 0)
    words, _ = eng.generate_rows(init, L, seed_len, K, np.repeat(np.arange(L, dtype=np.int32)[:, None], R, axis=1), hp,
                                 image_of_row=ior, snapshot_every=L, want_cos=False)
    rng = random.Random(11)
    blank_sets = [sorted(rng.sample(range(L), 1 + (r * 5 + 3) % L)) for r in range(R)]   # 1 .. 6 blanks, mixed over the rows
    assert len({len(b) for b in blank_sets}) > 2
    start = _blank_rows(su, words[-1], blank_sets)
    pos, n_mask, every = infill.infill_schedules(blank_sets, "shuffle", sweeps, rng=random.Random(12))
    return su, hp, ior, start, pos, every, L


def _pair_from(eng, start, L, pos, hp, ior, every, want_cos=True, n_mask=None):
    out = {}
    for on in (0, 1):
        eng.set_option("memo_rows", on)
        eng.profile_reset()
        ids, cos = eng.generate_rows_from(start, L, SEED_LEN, K, pos, hp, image_of_row=ior, n_mask=n_mask, snapshot_every=every,
                                          want_cos=want_cos)
        out[on] = (ids, cos, eng.stats(), eng.memo_rows_stats())
    eng.set_option("memo_rows", 0)
    return out


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_memo_rows_with_idle_steps_is_exact(prec):
    """Option "memo_rows" off against on over a schedule with idle steps, every step snapshotted: ids identical, cosine bits
    identical (CZC_PREC_REFINE as test_memo_rows_is_exact_on_a_converging_batch compares it: ids without cosines, then a
    per-sweep call within 1e-6); an idle step is neither a hit nor a counted row-step."""
    su, hp, ior, start, pos, every, L = _converging_infill(prec)
    eng = su.engine
    try:
        ran = int((pos != IDLE).sum())
        out = _pair_from(eng, start, L, pos, hp, ior, 1, want_cos=prec != REFINE)
        np.testing.assert_array_equal(out[0][0], out[1][0])
        if prec != REFINE:
            np.testing.assert_array_equal(_bits(out[0][1]), _bits(out[1][1]))
        print(f"[rows_from] prec {prec}: memo_rows {out[1][3]} of {ran} row-steps that are not idle ({pos.size} in all)")
        assert out[0][3] == dict(hit_row_steps=0, row_steps=0)
        assert out[1][3]["row_steps"] == ran and out[1][3]["hit_row_steps"] > 0
        assert out[0][2]["clip_seqs"] == K * ran
        assert out[1][2]["clip_seqs"] == K * (ran - out[1][3]["hit_row_steps"])
        if prec == REFINE:
            o2 = _pair_from(eng, start, L, pos, hp, ior, every)
            np.testing.assert_array_equal(o2[0][0], o2[1][0])
            np.testing.assert_allclose(o2[0][1], o2[1][1], rtol=0, atol=1e-6)
            assert o2[1][3]["hit_row_steps"] > 0
    finally:
        eng.close()


def test_span_groups_with_rows_idle_per_group():
    """L = 5, n_mask = [2, 0, 2, 0, 1] per sweep, rows idle for whole groups: option on against off, and against the czc_step
    chain (ids identical).  A row idle in half a group is refused."""
    L, R = 5, 6
    su, emb, init, hp = _tiny(F32, 2, L)
    eng = su.engine
    try:
        ior = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
        words, _ = eng.generate_rows(init, L, SEED_LEN, K, np.repeat(np.arange(L, dtype=np.int32)[:, None], R, axis=1), hp,
                                     image_of_row=ior, snapshot_every=L)
        start = words[-1].copy()
        takes = [(1, 1, 1), (1, 0, 1), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 0, 0)]   # per row: which of the three groups it runs
        sweep = np.full((5, R), IDLE, dtype=np.int32)
        for r, (g0, g1, g2) in enumerate(takes):
            if g0:
                sweep[0, r], sweep[1, r] = 0, 1
            if g1:
                sweep[2, r], sweep[3, r] = 2, 3
            if g2:
                sweep[4, r] = 4
        sweeps = 3
        pos = np.ascontiguousarray(np.tile(sweep, (sweeps, 1)))
        nm = [2, 0, 2, 0, 1] * sweeps
        eng.set_image_embeds(emb)
        out = _pair_from(eng, start, L, pos, hp, ior, 5, n_mask=nm)
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(_bits(out[0][1]), _bits(out[1][1]))
        assert out[1][3]["row_steps"] == int((pos != IDLE).sum())
        ref_ids, _ = _chain(eng, emb[ior], start, pos, nm, L, hp, 5)
        np.testing.assert_array_equal(out[0][0], ref_ids)
        np.testing.assert_array_equal(out[0][0][:, 5], np.broadcast_to(start[5], (sweeps, start.shape[1])))
        eng.set_image_embeds(emb)
        bad = pos.copy()
        bad[1, 0] = IDLE   # row 0 runs the n_mask = 2 step of its first group and sits the n_mask = 0 step out
        for on in (0, 1):
            eng.set_option("memo_rows", on)
            with pytest.raises(native.NativeError, match="whole step group") as ei:
                eng.generate_rows_from(start, L, SEED_LEN, K, bad, hp, image_of_row=ior, n_mask=nm, snapshot_every=5)
            assert ei.value.code == native.ERR_ARG
        eng.set_option("memo_rows", 0)
        ids, _ = eng.generate_rows_from(start, L, SEED_LEN, K, pos, hp, image_of_row=ior, n_mask=nm, snapshot_every=5)
        np.testing.assert_array_equal(ids, out[0][0])
    finally:
        eng.close()


def test_argument_checks_leave_the_engine_usable():
    L, R = 4, 3
    su, emb, init, hp = _tiny(F32, R, L)
    eng = su.engine
    try:
        start = np.tile(init, (R, 1))
        good = np.array([[0, 1, IDLE], [1, 0, 2], [3, IDLE, 3]], dtype=np.int32)
        want, _ = eng.generate_rows_from(start, L, SEED_LEN, K, good, hp, snapshot_every=3)

        def refused(match, rows=start, pos=good, hyper=hp):
            with pytest.raises(native.NativeError, match=match) as ei:
                eng.generate_rows_from(rows, L, SEED_LEN, K, pos, hyper, snapshot_every=3)
            assert ei.value.code == native.ERR_ARG
            ids, _ = eng.generate_rows_from(start, L, SEED_LEN, K, good, hp, snapshot_every=3)   # the engine is still usable
            np.testing.assert_array_equal(ids, want)

        bad = good.copy()
        bad[1, 1] = -2
        refused("position outside", pos=bad)
        bad = good.copy()
        bad[2, 2] = L
        refused("position outside", pos=bad)
        rows = start.copy()
        rows[1, 2] = su.bert_cfg.vocab
        refused("outside the BERT vocabulary", rows=rows)
        eng.set_lexicon(synth.make_lexicon(len(su.sv.bert_tokens)))
        eng.set_control_callback(lambda inp, cand, gen_idx: np.zeros(cand.shape, np.float32))
        try:
            with pytest.raises(native.NativeError, match="control callback") as ei:   # rows 0 and 1 at different positions
                eng.generate_rows_from(start, L, SEED_LEN, K, good, Engine.hyper(0.1, 2.0, 0.1, 0.5), snapshot_every=3)
            assert ei.value.code == native.ERR_ARG
        finally:
            eng.set_control_callback(None)
        ids, _ = eng.generate_rows_from(start, L, SEED_LEN, K, good, hp, snapshot_every=3)
        np.testing.assert_array_equal(ids, want)
        # czc_generate_rows keeps refusing an idle position
        with pytest.raises(native.NativeError, match="position out of range") as ei:
            eng.generate_rows(init, L, SEED_LEN, K, good, hp, snapshot_every=3)
        assert ei.value.code == native.ERR_ARG
        with pytest.raises(ValueError):
            eng.generate_rows_from(start[:2], L, SEED_LEN, K, good, hp, snapshot_every=3)
    finally:
        eng.close()


def test_a_host_scorer_sees_the_running_rows_compacted():
    """A controlled call with a callback whose rows that are not idle share one position per step: the callback's B is the
    running-row count at every step, and the result is the czc_step chain's with the same scorer."""
    L, R = 5, 6
    su, emb, init, hp0 = _tiny(F32, 2, L)
    eng = su.engine
    try:
        ior = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
        words, _ = eng.generate_rows(init, L, SEED_LEN, K, np.repeat(np.arange(L, dtype=np.int32)[:, None], R, axis=1), hp0,
                                     image_of_row=ior, snapshot_every=L)
        blank_sets = [[0, 1, 2, 3, 4], [1, 3], [0, 2, 4], [], [3, 4], [1, 2, 3]]
        start = _blank_rows(su, words[-1], blank_sets)
        order = [3, 1, 4, 0, 2]   # one shared order: row r runs the steps whose position is one of its blanks
        sweep = np.array([[p if p in bl else IDLE for bl in blank_sets] for p in order], dtype=np.int32)
        pos = np.ascontiguousarray(np.tile(sweep, (2, 1)))
        lex = synth.make_lexicon(len(su.sv.bert_tokens))
        eng.set_lexicon(lex)
        hp = Engine.hyper(0.1, 2.0, 0.1, 0.5)
        seen = []

        def scorer(inp, cand, gen_idx):
            seen.append((inp.shape[0], gen_idx))
            ctx = lex[inp].mean(axis=1, keepdims=True)
            return (lex[cand] + 0.25 * ctx).astype(np.float32)

        eng.set_control_callback(scorer)
        eng.set_image_embeds(emb)
        ids, cos = eng.generate_rows_from(start, L, SEED_LEN, K, pos, hp, image_of_row=ior, snapshot_every=L)
        assert [b for b, _ in seen] == [int(n) for n in (pos != IDLE).sum(axis=1)]
        assert [g for _, g in seen] == [SEED_LEN + p for p in order * 2]
        ref_ids, ref_cos = _chain(eng, emb[ior], start, pos, None, L, hp, L)
        np.testing.assert_array_equal(ids, ref_ids)
        np.testing.assert_allclose(cos, ref_cos, rtol=0, atol=1e-6)
    finally:
        eng.set_control_callback(None)
        eng.close()


def test_two_streams_return_the_single_engine_bits():
    L = 5
    su, emb, init, hp = _tiny(F32, 2, L)
    eng = su.engine
    try:
        ior, start, pos, n_mask, every, _ = _idle_case(su, emb, init, hp, L)
        eng.set_image_embeds(emb)
        ids0, cos0 = eng.generate_rows_from(start, L, SEED_LEN, K, pos, hp, image_of_row=ior, n_mask=n_mask, snapshot_every=every)
        grp = EngineGroup(eng, streams=2, min_images=3)
        try:
            grp.set_image_embeds(emb)
            ids1, cos1 = grp.generate_rows_from(start, L, SEED_LEN, K, pos, hp, image_of_row=ior, n_mask=n_mask,
                                                snapshot_every=every)
            assert len(grp.parts(6)) == 2
            np.testing.assert_array_equal(ids0, ids1)
            np.testing.assert_array_equal(_bits(cos0), _bits(cos1))
        finally:
            grp.close(parent=False)
    finally:
        eng.close()
