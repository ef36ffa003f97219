"""-m gpu: czc_generate_rows_draw (include/conzic_hip.h) -- a seeded draw of the winner per row.  Tiny synthetic towers, K = 200,
R <= 16 rows over two images, L <= 6, two sweeps.  The yardsticks: czc_generate_rows_hp for rows that do not draw, a host replay
of the call through czc_step and the NumPy reference of the draw (tests/draw_ref.py) for rows that do, and the call itself under
permutation, other companions, a split over streams and a resume for the independence properties."""
import random

import numpy as np
import pytest

import draw_ref as R
from conzic_amd import draws as D, harness, lengths, native
from conzic_amd.engine import Engine, EngineGroup

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT, REFINE = native.PREC_F32, native.PREC_BF16, native.PREC_SPLIT, native.PREC_REFINE
IDLE = native.POS_IDLE
K = 200
PROMPT = "Image of a"
SEED_LEN = 4
MIXED = [3, 6, 4, 6, 1, 5]
MIXED_IOR = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
HP = lambda: Engine.hyper(0.02, 2.0, 0.1)   # noqa: E731


def _tiny(prec, n_img=2):
    su = harness.build_synthetic(True, prec)
    emb = np.random.default_rng(3).standard_normal((n_img, su.clip_cfg.proj)).astype(np.float32)
    su.engine.set_image_embeds(emb)
    return su, emb


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _seeds(n, base=7):
    return [D.row_seed(base, 0, i) for i in range(n)]


def _mixed(su, sweeps=2, seed=1):
    start = lengths.length_rows(su.bert_tok, PROMPT, MIXED)
    pos, n_mask, _ = lengths.length_schedules(MIXED, "shuffle", sweeps, rng=random.Random(seed))
    return start, pos, n_mask


@pytest.mark.parametrize("memo", [0, 1])
@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_all_tau_zero_is_generate_rows_hp(prec, memo):
    """draws = None and draws whose taus are all 0: ids and cosine bits of czc_generate_rows_hp."""
    su, _ = _tiny(prec)
    eng = su.engine
    try:
        eng.set_option("memo_rows", memo)
        start, pos, n_mask = _mixed(su)
        hps = [Engine.hyper(0.02, (1.0, 2.0)[r % 2], 0.1) for r in range(6)]
        ids0, cos0 = eng.generate_rows_hp(start, MIXED, SEED_LEN, K, pos, hps, image_of_row=MIXED_IOR, n_mask=n_mask)
        for dr in (None, D.draw_rows(_seeds(6), 0.0, step0=5)):
            ids1, cos1 = eng.generate_rows_draw(start, MIXED, SEED_LEN, K, pos, hps, dr, image_of_row=MIXED_IOR, n_mask=n_mask)
            np.testing.assert_array_equal(ids0, ids1)
            np.testing.assert_array_equal(_bits(cos0), _bits(cos1))
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16])
def test_host_replay_with_the_reference_draw(prec):
    """Eight rows = eight images, L = 6, two sequential sweeps, tau 0.5 and 0.05 alternating: a loop of czc_step gives every
    step's final_score, probs and candidates, the reference draws the winner and writes it into the column; the one call returns
    the same ids.  A draw the reference calls a near tie follows the device's id (at most 1 % of the draws)."""
    n, L, sweeps = 8, 6, 2
    su, _ = _tiny(prec, n)
    eng = su.engine
    try:
        hp = HP()
        start = lengths.length_rows(su.bert_tok, PROMPT, [L] * n)
        pos, _, _ = lengths.length_schedules([L] * n, "sequential", sweeps)
        seeds = np.array(_seeds(n), dtype=np.uint64)
        taus = np.where(np.arange(n) % 2 == 0, 0.5, 0.05).astype(np.float32)
        ids, _ = eng.generate_rows_draw(start, None, SEED_LEN, K, pos, [HP() for _ in range(n)], R.make_draws(seeds, taus),
                                        snapshot_every=1)
        cur = np.ascontiguousarray(start, dtype=np.int32).copy()
        ties = moved = 0
        for s in range(pos.shape[0]):
            p = int(pos[s, 0])
            res = eng.step(cur, SEED_LEN + p, K, hp, dot_allowed=(p == L - 1), want=("probs", "cand_ids", "final_score", "best"))
            win, tie = R.winners(res["final_score"], res["probs"], seeds, taus, s)
            want = res["cand_ids"][np.arange(n), win]
            got = ids[s, :, SEED_LEN + p]
            bad = (got != want) & ~tie
            assert not bad.any(), (s, np.nonzero(bad)[0], got[bad], want[bad])
            ties += int(tie.sum())
            moved += int((win != res["best"]).sum())
            cur[:, SEED_LEN + p] = got          # (== want outside a near tie)
            np.testing.assert_array_equal(cur, ids[s])
        print(f"[rows_draw] replay prec {prec}: {n * pos.shape[0]} draws, {ties} near ties, {moved} winners off the argmax")
        assert ties <= R.NEAR_TIE_CAP * n * pos.shape[0]
        assert moved > 0
    finally:
        eng.close()


def _independence_batch(su):
    """Twelve rows over two images with mixed lengths and idle steps; rows 0 and 6 are twins (image, length, order, seed)."""
    lens = MIXED + MIXED
    ior = np.concatenate([MIXED_IOR, MIXED_IOR])
    start = lengths.length_rows(su.bert_tok, PROMPT, lens)
    pos, n_mask, _ = lengths.length_schedules(lens, "shuffle", 2, rng=random.Random(5))
    pos = pos.copy()
    pos[:, 6] = pos[:, 0]
    seeds = _seeds(12)
    seeds[6] = seeds[0]
    taus = [0.5] * 12
    return start, lens, ior, np.ascontiguousarray(pos), n_mask, seeds, taus


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_rows_are_independent(prec):
    """Twins return equal rows; permuting the rows permutes the ids; a row returns the same ids whether its companions draw, take
    the argmax or sit the call out; two streams return the single engine's ids.  Mixed lengths, idle steps."""
    su, emb = _tiny(prec)
    eng = su.engine
    try:
        start, lens, ior, pos, n_mask, seeds, taus = _independence_batch(su)
        hps = lambda n=12: [HP() for _ in range(n)]   # noqa: E731
        call = lambda st, ln, io, ps, sd, ta: eng.generate_rows_draw(st, ln, SEED_LEN, K, ps, hps(len(ln)), D.draw_rows(sd, ta),  # noqa: E731
                                                                     image_of_row=io, n_mask=n_mask)[0]
        ids = call(start, lens, ior, pos, seeds, taus)
        np.testing.assert_array_equal(ids[:, 0], ids[:, 6])
        assert (ids[:, 1] != ids[:, 7]).any()       # same image, length and hyper-parameters, another order and seed
        perm = np.random.default_rng(2).permutation(12)
        idsp = call(start[perm], [lens[i] for i in perm], ior[perm], np.ascontiguousarray(pos[:, perm]), [seeds[i] for i in perm],
                    [taus[i] for i in perm])
        np.testing.assert_array_equal(idsp, ids[:, perm])
        keep = [1, 3, 8]
        argmax = [t if r in keep else 0.0 for r, t in enumerate(taus)]
        np.testing.assert_array_equal(call(start, lens, ior, pos, seeds, argmax)[:, keep], ids[:, keep])
        idle = pos.copy()
        idle[:, [r for r in range(12) if r not in keep]] = IDLE
        np.testing.assert_array_equal(call(start, lens, ior, idle, seeds, taus)[:, keep], ids[:, keep])
        grp = EngineGroup(eng, streams=2, min_images=3)
        try:
            grp.set_image_embeds(emb)
            assert len(grp.parts(12)) == 2
            idsg, _ = grp.generate_rows_draw(start, lens, SEED_LEN, K, pos, hps(), D.draw_rows(seeds, taus), image_of_row=ior, n_mask=n_mask)
            np.testing.assert_array_equal(idsg, ids)
        finally:
            grp.close(parent=False)
            eng.set_image_embeds(emb)
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_tau_zero_rows_of_a_mixed_call(prec):
    """Every other row draws: the others return what czc_generate_rows_hp returns for them.  Ids identical; cosine bits identical
    on F32 / BF16, atol 1e-6 on SPLIT / REFINE (the rule of tests/test_generate_rows_hp_gpu.py)."""
    su, _ = _tiny(prec)
    eng = su.engine
    try:
        start, pos, n_mask = _mixed(su, seed=3)
        hps = [HP() for _ in range(6)]
        taus = [0.5 if r % 2 else 0.0 for r in range(6)]
        sel = [r for r in range(6) if taus[r] == 0.0]
        ids0, cos0 = eng.generate_rows_hp(start, MIXED, SEED_LEN, K, pos, hps, image_of_row=MIXED_IOR, n_mask=n_mask)
        ids1, cos1 = eng.generate_rows_draw(start, MIXED, SEED_LEN, K, pos, hps, D.draw_rows(_seeds(6), taus), image_of_row=MIXED_IOR,
                                            n_mask=n_mask)
        print(f"[rows_draw] mixed prec {prec}: max |d cos| {float(np.abs(cos0[:, sel] - cos1[:, sel]).max()):.3e}")
        np.testing.assert_array_equal(ids0[:, sel], ids1[:, sel])
        if prec in (F32, BF16):
            np.testing.assert_array_equal(_bits(cos0[:, sel]), _bits(cos1[:, sel]))
        else:
            np.testing.assert_allclose(cos0[:, sel], cos1[:, sel], rtol=0, atol=1e-6)
        assert (ids0 != ids1).any()
    finally:
        eng.close()


def test_seeds_matter_and_calls_repeat():
    """16 rows of one image, sequential order, tau = 10, distinct seeds: at least two distinct captions (under the argmax rule all
    16 are equal); the same call twice returns identical output."""
    su, _ = _tiny(BF16)
    eng = su.engine
    try:
        n, L = 16, 6
        start = lengths.length_rows(su.bert_tok, PROMPT, [L] * n)
        pos, _, _ = lengths.length_schedules([L] * n, "sequential", 2)
        ior = np.zeros(n, dtype=np.int32)
        hps = [HP() for _ in range(n)]
        dr = D.draw_rows(_seeds(n), 10.0)
        ids, cos = eng.generate_rows_draw(start, None, SEED_LEN, K, pos, hps, dr, image_of_row=ior)
        ids2, cos2 = eng.generate_rows_draw(start, None, SEED_LEN, K, pos, hps, dr, image_of_row=ior)
        np.testing.assert_array_equal(ids, ids2)
        np.testing.assert_array_equal(_bits(cos), _bits(cos2))
        assert len({ids[-1, r].tobytes() for r in range(n)}) >= 2
        ids0, _ = eng.generate_rows_hp(start, None, SEED_LEN, K, pos, hps, image_of_row=ior)
        assert len({ids0[-1, r].tobytes() for r in range(n)}) == 1
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16])
def test_resume_with_step0(prec):
    """One sweep, then one sweep from its snapshot with step0 = the steps already run, is the call over both sweeps."""
    su, _ = _tiny(prec)
    eng = su.engine
    try:
        n, L = 6, 6
        start = lengths.length_rows(su.bert_tok, PROMPT, [L] * n)
        pos, _, _ = lengths.length_schedules([L] * n, "shuffle", 2, rng=random.Random(4))
        hps = [HP() for _ in range(n)]
        seeds = _seeds(n)
        ids, _ = eng.generate_rows_draw(start, None, SEED_LEN, K, pos, hps, D.draw_rows(seeds, 0.5), image_of_row=MIXED_IOR)
        a, _ = eng.generate_rows_draw(start, None, SEED_LEN, K, pos[:L], hps, D.draw_rows(seeds, 0.5), image_of_row=MIXED_IOR)
        b, _ = eng.generate_rows_draw(a[-1], None, SEED_LEN, K, pos[L:], hps, D.draw_rows(seeds, 0.5, step0=L), image_of_row=MIXED_IOR)
        np.testing.assert_array_equal(a[-1], ids[0])
        np.testing.assert_array_equal(b[-1], ids[1])
        c, _ = eng.generate_rows_draw(a[-1], None, SEED_LEN, K, pos[L:], hps, D.draw_rows(seeds, 0.5), image_of_row=MIXED_IOR)
        assert (c[-1] != ids[1]).any()      # without the offset the second sweep repeats the first sweep's noise
    finally:
        eng.close()


def test_memo_rows_serves_only_the_rows_that_do_not_draw():
    """The converging setup of tests/test_memo_rows_gpu.py, four images x four rows, eight shuffle sweeps; rows 0, 3, 6, ... draw
    (tau = 0.02).  Option on returns the ids of option off; the hits are the rule's on the rows that do not draw, and none
    comes from a row that draws."""
    B, S, L, sweeps = 4, 4, 6, 8
    n = B * S
    su, _, hp, init, seed_len = harness.converging_setup(B=B, L=L, precision=BF16)
    eng = su.engine
    try:
        cols = []
        rng = random.Random(5)
        for _ in range(n):
            o = list(range(L))
            rng.shuffle(o)
            cols.append(harness.order_positions("shuffle", L, sweeps, order_list=o)[0])
        pos = np.ascontiguousarray(np.array(cols, dtype=np.int32).T)
        ior = np.tile(np.arange(B, dtype=np.int32), S)
        start = np.ascontiguousarray(np.repeat(init[None, :], n, axis=0))
        taus = np.array([0.02 if r % 3 == 0 else 0.0 for r in range(n)])
        hps = [Engine.hyper(hp.alpha, hp.beta, hp.temperature) for _ in range(n)]
        dr = D.draw_rows(_seeds(n), taus.tolist())
        out = {}
        for on in (0, 1):
            eng.set_option("memo_rows", on)
            eng.profile_reset()
            ids, _ = eng.generate_rows_draw(start, None, seed_len, K, pos, hps, dr, image_of_row=ior, snapshot_every=1)
            out[on] = (ids, eng.memo_rows_stats())
        np.testing.assert_array_equal(out[0][0], out[1][0])
        exp = harness.memo_expected_hits_rows(out[0][0], pos, None, seed_len, su.bert_tok.vocab["[MASK]"])
        print(f"[rows_draw] memo_rows {out[1][1]}; rule: {int(exp[:, taus == 0].sum())} hits on argmax rows, "
              f"{int(exp[:, taus > 0].sum())} refused on drawing rows")
        assert out[0][1] == dict(hit_row_steps=0, row_steps=0)
        assert exp[:, taus == 0].sum() > 0
        assert out[1][1] == dict(hit_row_steps=int(exp[:, taus == 0].sum()), row_steps=n * pos.shape[0])
    finally:
        eng.close()


def test_refine_engine_never_gates_a_row_that_draws():
    """CZC_PREC_REFINE, every row draws: the second pass ran, no image-step was gated, the guard is not tripped; with the same
    rows under the argmax rule the gate does see image-steps."""
    su, _ = _tiny(REFINE)
    eng = su.engine
    try:
        start, pos, n_mask = _mixed(su, seed=6)
        hps = [HP() for _ in range(6)]
        eng.refine_guard(reset=True)
        eng.profile_reset()
        eng.generate_rows_draw(start, MIXED, SEED_LEN, K, pos, hps, D.draw_rows(_seeds(6), 0.5), image_of_row=MIXED_IOR, n_mask=n_mask)
        st, guard = eng.stats(), eng.refine_guard(reset=True)
        print(f"[rows_draw] refine, all rows draw: {st['refine_seqs']} re-encoded, {st['gated_image_steps']} of {st['gate_image_steps']} gated, guard {guard}")
        assert st["refine_seqs"] > 0 and st["gated_image_steps"] == 0 and st["gate_image_steps"] == 0
        assert guard["tripped"] == 0
        eng.profile_reset()
        eng.generate_rows_hp(start, MIXED, SEED_LEN, K, pos, hps, image_of_row=MIXED_IOR, n_mask=n_mask)
        assert eng.stats()["gate_image_steps"] > 0
    finally:
        eng.close()


def test_bad_arguments_leave_the_engine_usable():
    su, _ = _tiny(F32)
    eng = su.engine
    try:
        start, pos, n_mask = _mixed(su)
        hps = [HP() for _ in range(6)]
        good = D.draw_rows(_seeds(6), 0.5)
        want, _ = eng.generate_rows_draw(start, MIXED, SEED_LEN, K, pos, hps, good, image_of_row=MIXED_IOR, n_mask=n_mask)
        eng.profile_reset()

        def refused(match, **kw):
            bad = D.draw_rows(_seeds(6), 0.5)
            for k, v in kw.items():
                setattr(bad[2], k, v)
            with pytest.raises(native.NativeError, match=match) as ei:
                eng.generate_rows_draw(start, MIXED, SEED_LEN, K, pos, hps, bad, image_of_row=MIXED_IOR, n_mask=n_mask)
            assert ei.value.code == native.ERR_ARG
            assert eng.stats()["steps"] == 0   # refused before any GPU work
            ids, _ = eng.generate_rows_draw(start, MIXED, SEED_LEN, K, pos, hps, good, image_of_row=MIXED_IOR, n_mask=n_mask)
            np.testing.assert_array_equal(ids, want)
            eng.profile_reset()

        refused("tau", tau=-0.5)
        refused("tau", tau=float("nan"))
        refused("tau", tau=float("inf"))
        refused("step counter", step0=2 ** 32 - pos.shape[0])
        edge = D.draw_rows(_seeds(6), 0.5, step0=2 ** 32 - 1 - pos.shape[0])   # step0 + n_steps = 2^32 - 1: fits
        eng.generate_rows_draw(start, MIXED, SEED_LEN, K, pos, hps, edge, image_of_row=MIXED_IOR, n_mask=n_mask)
        with pytest.raises(ValueError):
            eng.generate_rows_draw(start, MIXED, SEED_LEN, K, pos, hps, good[:5], image_of_row=MIXED_IOR, n_mask=n_mask)
    finally:
        eng.close()
