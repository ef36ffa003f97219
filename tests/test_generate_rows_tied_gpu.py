"""-m gpu: czc_generate_rows_tied (include/conzic_hip.h) -- rows tied into groups that hold one sentence, so that the W slots of a
caption polish W positions per step.  Tiny synthetic towers, K = 200, at most 18 rows, two sweeps.  The yardsticks:
czc_generate_rows_draw for untied rows; a host chain of one-step czc_generate_rows_draw calls whose winners are merged within
the groups in NumPy; Engine.score_rows for the merged captions' cosines; a Jacobi chain of oracle.step.polish_step on F32."""
import numpy as np
import pytest
import torch

from conzic_amd import blocks as B, draws as D, harness, lengths, native, synth
from conzic_amd.engine import Engine

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT, REFINE = native.PREC_F32, native.PREC_BF16, native.PREC_SPLIT, native.PREC_REFINE
IDLE = native.POS_IDLE
K = 200
PROMPT = "Image of a"
SEED_LEN = 4
HP = lambda: Engine.hyper(0.02, 2.0, 0.1)   # noqa: E731
# "one sentence in another packing": the cos_tol of tests/test_step_gpu.py::test_dedup_is_exact
PACK_TOL = {F32: 2e-6, SPLIT: 2e-6, BF16: 1e-3, REFINE: 4e-4}


def _tiny(prec, n_img=2):
    su = harness.build_synthetic(True, prec)
    emb = np.random.default_rng(3).standard_normal((n_img, su.clip_cfg.proj)).astype(np.float32)
    su.engine.set_image_embeds(emb)
    return su, emb


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _schedule(lens, width, layout, sweeps):
    """Tied rows of len(lens) captions with `width` slots each: (positions [n_steps, R], snapshot_every, groups, lens per row).
    Every sweep takes max over the captions of ceil(L / width) steps; a caption with fewer blocks idles for the rest of it."""
    nbm = max(B.n_blocks(n, width) for n in lens)
    per = []
    for n in lens:
        one, nb = B.tied_positions([B.sequential_order(n, width, layout)] * sweeps, width)
        one = one.reshape(sweeps, nb, width)
        pad = np.full((sweeps, nbm - nb, width), IDLE, dtype=np.int32)
        per.append(np.concatenate([one, pad], axis=1).reshape(sweeps * nbm, width))
    groups, cap, _ = B.tied_rows(len(lens), width)
    return B.caption_positions(per), nbm, groups, [lens[c] for c in cap]


def _merge(new, old, pos, groups):
    """The tie on the host: every row that ran hands the id in its column to the other rows of its group."""
    out = new.copy()
    for r in range(new.shape[0]):
        if pos[r] == IDLE:
            continue
        c = SEED_LEN + int(pos[r])
        out[groups == groups[r], c] = new[r, c]
    return out


def _chain(eng, start, lens, ior, pos, hps, seeds, taus, groups):
    """One czc_generate_rows_draw call of one step per step on the current rows (step0 = s), winners merged within groups."""
    cur = np.ascontiguousarray(start, dtype=np.int32).copy()
    snaps = []
    for s in range(pos.shape[0]):
        dr = None if seeds is None else D.draw_rows(seeds, taus, step0=s)
        ids, _ = eng.generate_rows_draw(cur, lens, SEED_LEN, K, pos[s:s + 1], hps, dr, image_of_row=ior, snapshot_every=1,
                                        want_cos=False)
        cur = _merge(ids[0], cur, pos[s], groups)
        snaps.append(cur.copy())
    return np.stack(snaps)


def _leader_scores(eng, rows, groups, lens, ior):
    """Engine.score_rows of the rows, one row per group as the tied call scores them, handed to every member."""
    lead = np.array([int(np.nonzero(groups == g)[0][0]) for g in groups])
    uniq = np.unique(lead)
    sc = eng.score_rows(rows[uniq], SEED_LEN, None if lens is None else [lens[i] for i in uniq], ior[uniq])
    return sc[np.searchsorted(uniq, lead)]


@pytest.mark.parametrize("prec", [F32, BF16])
def test_no_groups_is_generate_rows_draw(prec):
    su, _ = _tiny(prec)
    eng = su.engine
    try:
        lens = [3, 6, 4, 6, 1, 5]
        ior = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
        start = lengths.length_rows(su.bert_tok, PROMPT, lens)
        pos, _, _ = lengths.length_schedules(lens, "sequential", 2)
        hps = [HP() for _ in lens]
        dr = D.draw_rows([D.row_seed(7, 0, i) for i in range(6)], [0.5, 0.0] * 3)
        ids0, cos0 = eng.generate_rows_draw(start, lens, SEED_LEN, K, pos, hps, dr, image_of_row=ior)
        ids1, cos1 = eng.generate_rows_tied(start, lens, SEED_LEN, K, pos, hps, dr, None, image_of_row=ior)
        np.testing.assert_array_equal(ids0, ids1)
        np.testing.assert_array_equal(_bits(cos0), _bits(cos1))
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_singleton_groups(prec):
    """Every row a group of its own (ids in any order inside [0, R)): the ids of czc_generate_rows_draw bit for bit; the cosines
    -- now czc_score_rows of the row as it stands, which for an untied row is the winner's sentence -- within the bar for one
    sentence in another packing."""
    su, _ = _tiny(prec)
    eng = su.engine
    try:
        lens = [3, 6, 4, 6, 1, 5]
        ior = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
        start = lengths.length_rows(su.bert_tok, PROMPT, lens)
        pos, _, _ = lengths.length_schedules(lens, "sequential", 2)
        hps = [HP() for _ in lens]
        ids0, cos0 = eng.generate_rows_draw(start, lens, SEED_LEN, K, pos, hps, None, image_of_row=ior)
        ids1, cos1 = eng.generate_rows_tied(start, lens, SEED_LEN, K, pos, hps, None, [5, 3, 0, 1, 4, 2], image_of_row=ior)
        np.testing.assert_array_equal(ids0, ids1)
        err = float(np.abs(cos0.astype(np.float64) - cos1).max())
        print(f"[rows_tied] singleton groups prec {prec}: worst |d cos| against the winner cosines {err:.3e} (bar {PACK_TOL[prec]:.0e})")
        assert err <= PACK_TOL[prec]
    finally:
        eng.close()


CASES = {
    "w3_interleaved": (3, "interleaved", [6, 6, 6], False),
    "w4_contiguous": (4, "contiguous", [6, 6, 6], False),     # short last block: idle rows, compact batches
    "w6": (6, "interleaved", [6, 6, 6], False),
    "mixed_lengths": (4, "contiguous", [6, 4, 5], False),
    "some_rows_draw": (3, "interleaved", [6, 6, 6], True),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_equals_the_chain_of_existing_calls(prec, case):
    """Three captions over two images, two sweeps.  Ids equal the chain's at every snapshot (here: every step); the merged
    cosines equal Engine.score_rows of the chain's rows within 2e-6.  (CZC_PREC_REFINE: ids and these cosines; no cosine bits
    are compared on any precision.)"""
    width, layout, lens, draw = CASES[case]
    su, _ = _tiny(prec)
    eng = su.engine
    try:
        pos, nb, groups, row_lens = _schedule(lens, width, layout, 2)
        R = pos.shape[1]
        img_of_cap = np.array([0, 1, 0], dtype=np.int32)
        ior = np.ascontiguousarray(img_of_cap[groups])
        uniform = len(set(lens)) == 1
        start = lengths.length_rows(su.bert_tok, PROMPT, row_lens)
        ln = None if uniform else row_lens
        hps = [Engine.hyper(0.02, (2.0, 1.5)[r % 2], 0.1) for r in range(R)]
        seeds = [D.row_seed(11, int(groups[r]), 0, r % width) for r in range(R)] if draw else None
        taus = [0.5 if r % 3 != 1 else 0.0 for r in range(R)] if draw else None
        dr = D.draw_rows(seeds, taus) if draw else None
        ids, cos = eng.generate_rows_tied(start, ln, SEED_LEN, K, pos, hps, dr, groups, image_of_row=ior, snapshot_every=1)
        ref = _chain(eng, start, ln, ior, pos, hps, seeds, taus, groups)
        np.testing.assert_array_equal(ids, ref)
        assert (ids[-1] != start).any()
        worst = 0.0
        for s in range(pos.shape[0]):
            want = _leader_scores(eng, ref[s], groups, ln, ior)
            worst = max(worst, float(np.abs(cos[s].astype(np.float64) - want).max()))
        print(f"[rows_tied] chain {case} prec {prec}: {pos.shape[0]} steps, {R} rows, worst |d merged cos| {worst:.3e}")
        assert worst <= 2e-6
        # per sweep snapshots of the same call: the rows after every nb-th step
        ids2, cos2 = eng.generate_rows_tied(start, ln, SEED_LEN, K, pos, hps, dr, groups, image_of_row=ior, snapshot_every=nb)
        np.testing.assert_array_equal(ids2, ids[nb - 1::nb])
        assert float(np.abs(cos2.astype(np.float64) - cos[nb - 1::nb]).max()) <= 2e-6
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_group_members_agree_after_every_step(prec):
    """snapshot_every = 1, groups that are not contiguous and carry arbitrary ids: after every step all rows of a group hold
    identical ids and identical cosine bits."""
    su, _ = _tiny(prec)
    eng = su.engine
    try:
        pos, nb, groups, row_lens = _schedule([6, 6, 6], 4, "interleaved", 2)
        R = pos.shape[1]
        perm = np.random.default_rng(4).permutation(R)
        gid = np.array([9, 2, 11], dtype=np.int32)[groups][perm]       # arbitrary ids in [0, R), rows of a group scattered
        ior = np.array([0, 1, 0], dtype=np.int32)[groups][perm]
        pos = np.ascontiguousarray(pos[:, perm])
        start = lengths.length_rows(su.bert_tok, PROMPT, row_lens)
        ids, cos = eng.generate_rows_tied(start, None, SEED_LEN, K, pos, [HP() for _ in range(R)], None, gid, image_of_row=ior,
                                          snapshot_every=1)
        assert ids.shape[0] == pos.shape[0]
        for g in np.unique(gid):
            m = np.nonzero(gid == g)[0]
            for s in range(ids.shape[0]):
                assert (ids[s, m] == ids[s, m[0]]).all(), (g, s)
                assert (_bits(cos[s, m]) == _bits(cos[s, m[0]])).all(), (g, s)
        assert len({ids[-1, np.nonzero(gid == g)[0][0]].tobytes() for g in np.unique(gid)}) > 1
    finally:
        eng.close()


@pytest.mark.parametrize("width", [5, 2])
def test_f32_against_a_jacobi_chain_of_the_cpu_oracle(width):
    """Two captions (two images), L = 5, two sweeps, interleaved blocks.  For each position of a block: copy the old sentence,
    mask the position, take oracle.step.polish_step's winner; then write all winners.  Ids equal; the merged cosine within 2e-5
    (the bound of the trajectory goldens) of the oracle's cosine of the merged sentence."""
    from oracle import models as M, step as S, text as T
    L, sweeps = 5, 2
    su, emb = _tiny(F32)
    eng = su.engine
    try:
        sv = su.sv
        o = S.Oracle(M.to_torch(synth.make_bert_weights(su.bert_cfg, 11)), su.bert_cfg,
                     M.to_torch(synth.make_clip_weights(su.clip_cfg, 12)), su.clip_cfg, sv.bert_tokens,
                     T.ClipBpe(sv.clip_vocab, sv.clip_merges))
        pos, nb, groups, row_lens = _schedule([L, L], width, "interleaved", sweeps)
        start = lengths.length_rows(su.bert_tok, PROMPT, row_lens)
        ids, cos = eng.generate_rows_tied(start, None, SEED_LEN, K, pos, [HP() for _ in groups], None, groups, image_of_row=groups,
                                          snapshot_every=nb)
        blocks = B.sequential_order(L, width, "interleaved")
        worst = 0.0
        for c in range(2):
            cur = torch.tensor(o.init_text(PROMPT, L, 1))
            img = torch.from_numpy(emb[c:c + 1])
            for sw in range(sweeps):
                for block in blocks:
                    new = cur.clone()
                    for p in block:
                        inp = cur.clone()
                        inp[:, SEED_LEN + p] = o.mask_id
                        tmask = torch.from_numpy(su.token_mask.copy())
                        o.update_token_mask(tmask, L, p)
                        S.polish_step(o, inp, img, tmask, SEED_LEN + p, K, 0.1, 0.02, 2.0)
                        new[:, SEED_LEN + p] = inp[:, SEED_LEN + p]
                    cur = new
                te = o.text_embeds([o.decode(cur[0])]).double().numpy()[0]
                ie = emb[c].astype(np.float64)
                want = float(te @ ie / np.linalg.norm(te) / np.linalg.norm(ie))
                for r in np.nonzero(groups == c)[0]:
                    np.testing.assert_array_equal(ids[sw, r], cur[0].numpy())
                    worst = max(worst, abs(float(cos[sw, r]) - want))
        print(f"[rows_tied] oracle Jacobi chain width {width}: worst |d merged cos| {worst:.3e}")
        assert worst <= 2e-5
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [BF16, REFINE])
def test_memo_rows_is_exact(prec):
    """harness.converging_setup, two captions of three slots, eight sweeps: option "memo_rows" on returns the ids of the option
    off; on BF16 czc_memo_rows_stats shows hits (a row that hit still hands its restored winner to its siblings)."""
    su, _, hp, init, seed_len = harness.converging_setup(B=2, L=6, precision=prec)
    assert seed_len == SEED_LEN
    eng = su.engine
    try:
        one, nb = B.tied_positions([B.sequential_order(6, 3, "interleaved")] * 8, 3)
        pos = B.caption_positions([one, one])
        groups, _, ior = B.tied_rows(2, 3)
        start = np.repeat(np.asarray(init, dtype=np.int32)[None, :], 6, axis=0)
        out = []
        for memo in (0, 1):
            eng.set_option("memo_rows", memo)
            eng.profile_reset()
            ids, cos = eng.generate_rows_tied(start, None, SEED_LEN, K, pos, [hp] * 6, None, groups, image_of_row=ior, snapshot_every=1)
            out.append((ids, cos, eng.memo_rows_stats()))
        np.testing.assert_array_equal(out[0][0], out[1][0])
        assert float(np.abs(out[0][1].astype(np.float64) - out[1][1]).max()) <= 2e-6   # the same rows through czc_score_rows
        print(f"[rows_tied] memo_rows prec {prec}: {out[1][2]}")
        assert out[0][2] == dict(hit_row_steps=0, row_steps=0)
        assert out[1][2]["row_steps"] == pos.size
        if prec == BF16:
            assert out[1][2]["hit_row_steps"] > 0
    finally:
        eng.set_option("memo_rows", 0)
        eng.close()


def test_argument_errors_leave_the_engine_usable():
    su, _ = _tiny(F32)
    eng = su.engine
    try:
        pos, nb, groups, row_lens = _schedule([6, 6], 3, "interleaved", 1)
        R = pos.shape[1]
        ior = np.ascontiguousarray(groups)
        start = lengths.length_rows(su.bert_tok, PROMPT, row_lens)
        hps = [HP() for _ in range(R)]
        good, _ = eng.generate_rows_tied(start, None, SEED_LEN, K, pos, hps, None, groups, image_of_row=ior, snapshot_every=nb)
        assert good.shape[0] == 1

        def refused(st=start, ln=None, ps=pos, gr=groups, io=ior, n_mask=None):
            with pytest.raises(native.NativeError) as ei:
                if n_mask is None:
                    eng.generate_rows_tied(st, ln, SEED_LEN, K, ps, hps, None, gr, image_of_row=io, snapshot_every=nb)
                else:   # the Python method always passes n_mask = NULL (every step masks one position): the C ABI directly
                    st_, ps_ = np.ascontiguousarray(st, np.int32), np.ascontiguousarray(ps, np.int32)
                    nm, gr_, io_ = np.asarray(n_mask, np.int32), np.asarray(gr, np.int32), np.asarray(io, np.int32)
                    ids = np.empty((1, R, st_.shape[1]), np.int32)
                    from conzic_amd.engine import hyper_array
                    rc = eng.lib.czc_generate_rows_tied(eng.h, R, st_.shape[1], SEED_LEN, st_.ctypes.data, None, io_.ctypes.data,
                                                        gr_.ctypes.data, K, ps_.shape[0], ps_.ctypes.data, nm.ctypes.data, nb,
                                                        hyper_array(hps), None, ids.ctypes.data, None)
                    eng._ck(rc, "czc_generate_rows_tied")
            assert ei.value.code == native.ERR_ARG, ei.value
            again, _ = eng.generate_rows_tied(start, None, SEED_LEN, K, pos, hps, None, groups, image_of_row=ior, snapshot_every=nb)
            np.testing.assert_array_equal(again, good)

        other = start.copy()
        other[1, SEED_LEN + 2] = int(np.nonzero(su.token_mask[0] > 0)[0][0])
        refused(st=other)                                                   # start rows differ inside a group
        short = lengths.length_rows(su.bert_tok, PROMPT, [6, 6, 5, 6, 6, 6])
        short_pos = pos.copy()
        short_pos[short_pos[:, 2] >= 5, 2] = IDLE
        refused(st=short, ln=[6, 6, 5, 6, 6, 6], ps=short_pos)              # lengths differ inside a group
        refused(io=np.array([0, 0, 1, 1, 1, 1], dtype=np.int32))            # images differ inside a group
        clash = pos.copy()
        clash[0, 1] = clash[0, 0]
        refused(ps=clash)                                                   # two members on one column at a step
        refused(n_mask=[0] * pos.shape[0])
        refused(n_mask=[2] + [1] * (pos.shape[0] - 1))
        for bad in (R, -1):
            gr = groups.copy()
            gr[3] = bad
            refused(gr=gr)                                                  # a group id outside [0, R)
    finally:
        eng.close()
