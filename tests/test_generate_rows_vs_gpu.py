"""-m gpu: czc_generate_rows_vs / czc_score_rows_vs (include/conzic_hip.h) -- rows scored against rival images of the resident
batch.  Tiny synthetic towers, K = 200, at most 8 rows of lengths 1..6, 3 resident images, two sweeps.  The yardsticks:
czc_generate_rows_tied for everything without rivals (bits); the rows' own permutations; and, teacher-forced step by step, the CPU
oracle's polish_step with delta * disc_ref added in float64."""
import numpy as np
import pytest
import torch

from conzic_amd import draws as D, harness, lengths, native, rivals, synth
from conzic_amd.engine import Engine
from oracle import text as T

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT, REFINE = native.PREC_F32, native.PREC_BF16, native.PREC_SPLIT, native.PREC_REFINE
IDLE = native.POS_IDLE
K = 200
PROMPT = "Image of a"
SEED_LEN = 4
N_IMG = 3
LENS = [3, 6, 4, 6, 1, 5, 2, 6]
IOR = np.array([0, 1, 2, 0, 1, 2, 0, 1], dtype=np.int32)
DELTAS = np.array([1.0, 0.0, 0.5, 2.0, 1.0, 0.0, 0.5, 1.0], dtype=np.float32)   # rows 1 and 5: delta = 0
# tests/test_step_gpu.py::tol_final, restated for the two exact precisions the oracle test runs on
TOL_FINAL = {F32: 2e-5, SPLIT: 1e-4}
# oracle chain (tests run it on the CPU; seeds and deltas were chosen with it): see test_teacher_forced_against_the_cpu_oracle
ORACLE_LENS = [3, 6, 4, 1, 5, 2]
ORACLE_IOR = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
ORACLE_DELTAS = np.array([1.0, 2.0, 0.5, 1.0, 2.0, 0.0], dtype=np.float32)


def HP():
    return Engine.hyper(0.02, 2.0, 0.1)


def _tiny(prec, logit_scale=2.6592):
    su = harness.build_synthetic(True, prec, logit_scale=logit_scale)
    emb = np.random.default_rng(3).standard_normal((N_IMG, su.clip_cfg.proj)).astype(np.float32)
    su.engine.set_image_embeds(emb)
    return su, emb


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _table(emb, ior, M=2):
    return rivals.expand(rivals.rival_table(emb, M), ior)


def _call(su, lens=LENS, ior=IOR, sweeps=2):
    start = lengths.length_rows(su.bert_tok, PROMPT, lens)
    pos, _, every = lengths.length_schedules(lens, "sequential", sweeps)
    return start, pos, every, [HP() for _ in lens]


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_no_rivals_is_generate_rows_tied(prec):
    """rival_of_row = None, all-zero deltas and a table without a filled slot: the ids and cosine bits of generate_rows_tied."""
    su, emb = _tiny(prec)
    eng = su.engine
    try:
        start, pos, every, hps = _call(su)
        dr = D.draw_rows([D.row_seed(7, 0, i) for i in range(len(LENS))], [0.5, 0.0] * 4)
        ids0, cos0 = eng.generate_rows_tied(start, LENS, SEED_LEN, K, pos, hps, dr, None, image_of_row=IOR)
        tab = _table(emb, IOR)
        for rv, dl in ((None, DELTAS), (tab, np.zeros(len(LENS), np.float32)), (np.full_like(tab, -1), DELTAS)):
            ids1, cos1 = eng.generate_rows_vs(start, LENS, SEED_LEN, K, pos, hps, dr, None, rv, dl, image_of_row=IOR)
            np.testing.assert_array_equal(ids0, ids1)
            np.testing.assert_array_equal(_bits(cos0), _bits(cos1))
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16])
def test_mixed_call_leaves_the_rows_without_the_term_alone(prec):
    """Rows with delta = 0 (1 and 5) and a row without a rival (7) return the bits they have in the rival-free call; the call as
    a whole does not (the term acts on the others)."""
    su, emb = _tiny(prec)
    eng = su.engine
    try:
        start, pos, every, hps = _call(su)
        tab = _table(emb, IOR)
        tab[7, :] = -1
        ids0, cos0 = eng.generate_rows_tied(start, LENS, SEED_LEN, K, pos, hps, None, None, image_of_row=IOR, snapshot_every=1)
        ids1, cos1 = eng.generate_rows_vs(start, LENS, SEED_LEN, K, pos, hps, None, None, tab, DELTAS, image_of_row=IOR, snapshot_every=1)
        for r in (1, 5, 7):
            np.testing.assert_array_equal(ids0[:, r], ids1[:, r])
            np.testing.assert_array_equal(_bits(cos0[:, r]), _bits(cos1[:, r]))
        assert (ids0 != ids1).any()
    finally:
        eng.close()


@pytest.mark.parametrize("prec", [F32, BF16])
def test_rows_are_independent_of_their_index(prec):
    """Permuting the rows with their records (start row, length, schedule, hyper-parameters, draw, image, rivals, delta)
    permutes ids and cosine bits."""
    su, emb = _tiny(prec)
    eng = su.engine
    try:
        start, pos, every, hps = _call(su)
        tab = _table(emb, IOR)
        dr = D.draw_rows([D.row_seed(9, 0, i) for i in range(len(LENS))], [0.0, 0.5] * 4)
        ids0, cos0 = eng.generate_rows_vs(start, LENS, SEED_LEN, K, pos, hps, dr, None, tab, DELTAS, image_of_row=IOR)
        perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
        ids1, cos1 = eng.generate_rows_vs(start[perm], [LENS[i] for i in perm], SEED_LEN, K, np.ascontiguousarray(pos[:, perm]),
                                          [hps[i] for i in perm], [dr[i] for i in perm], None, tab[perm], DELTAS[perm],
                                          image_of_row=IOR[perm])
        np.testing.assert_array_equal(ids0[:, perm], ids1)
        np.testing.assert_array_equal(_bits(cos0[:, perm]), _bits(cos1))
    finally:
        eng.close()


def test_idle_rows_equal_the_rows_run_alone():
    """The mixed-length schedule idles the short rows (the compact-batch path gathers the rival tables through the run list):
    every row returns what it returns in a call of its own."""
    su, emb = _tiny(BF16)
    eng = su.engine
    try:
        start, pos, every, hps = _call(su)
        assert (pos == IDLE).any()
        tab = _table(emb, IOR)
        ids0, cos0 = eng.generate_rows_vs(start, LENS, SEED_LEN, K, pos, hps, None, None, tab, DELTAS, image_of_row=IOR)
        for r in (0, 3, 4, 6):
            n = LENS[r]
            st = lengths.length_rows(su.bert_tok, PROMPT, [n])
            ps, _, ev = lengths.length_schedules([n], "sequential", 2)
            ids1, cos1 = eng.generate_rows_vs(st, [n], SEED_LEN, K, ps, [hps[r]], None, None, tab[r:r + 1], DELTAS[r:r + 1],
                                              image_of_row=IOR[r:r + 1])
            np.testing.assert_array_equal(ids0[:, r, :st.shape[1]], ids1[:, 0])
            np.testing.assert_array_equal(_bits(cos0[:, r]), _bits(cos1[:, 0]))
    finally:
        eng.close()


def test_memo_rows_is_exact():
    """harness.converging_setup, six rows over three images, eight sweeps: option "memo_rows" on returns the ids and cosines of
    the option off, and czc_memo_rows_stats shows hits."""
    su, emb, hp, init, seed_len = harness.converging_setup(B=N_IMG, L=6, precision=BF16)
    assert seed_len == SEED_LEN
    eng = su.engine
    try:
        R = 6
        ior = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
        pos = np.ascontiguousarray(np.tile(np.arange(6, dtype=np.int32)[:, None], (8, R)))
        start = np.repeat(np.asarray(init, dtype=np.int32)[None, :], R, axis=0)
        tab = _table(emb, ior)
        dl = np.array([0.5, 1.0, 0.0, 1.0, 0.5, 2.0], np.float32)
        out = []
        for memo in (0, 1):
            eng.set_option("memo_rows", memo)
            eng.profile_reset()
            ids, cos = eng.generate_rows_vs(start, None, SEED_LEN, K, pos, [hp] * R, None, None, tab, dl, image_of_row=ior)
            out.append((ids, cos, eng.memo_rows_stats()))
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(_bits(out[0][1]), _bits(out[1][1]))
        print(f"[rows_vs] memo_rows: {out[1][2]}")
        assert out[1][2]["row_steps"] == pos.size and out[1][2]["hit_row_steps"] > 0
    finally:
        eng.set_option("memo_rows", 0)
        eng.close()


# ---- teacher-forced against the CPU oracle ------------------------------------------------------------------------------------
_ORACLE_CACHE = {}


def make_oracle(su):
    from oracle import models as M, step as S
    sv = su.sv
    return S.Oracle(M.to_torch(synth.make_bert_weights(su.bert_cfg, 11)), su.bert_cfg,
                    M.to_torch(synth.make_clip_weights(su.clip_cfg, 12)), su.clip_cfg, sv.bert_tokens,
                    T.ClipBpe(sv.clip_vocab, sv.clip_merges))


def oracle_row_step(o, token_mask, row, n, p, emb, own, rivals_of_row, delta, scale):
    """One row-step of the reference with the rival term: `row` int [T_r] before the step, position p of n.  Returns (winner id
    with the term, winner id without it, top-2 margin of the scores with the term)."""
    from oracle import step as S
    key = (row.tobytes(), n, p, own, tuple(int(v) for v in rivals_of_row), float(delta))
    if key in _ORACLE_CACHE:
        return _ORACLE_CACHE[key]
    inp = torch.from_numpy(row[:SEED_LEN + n + 1].astype(np.int64))[None, :].clone()
    inp[:, SEED_LEN + p] = o.mask_id
    tmask = torch.from_numpy(token_mask.copy())
    o.update_token_mask(tmask, n, p)
    r = S.polish_step(o, inp, torch.from_numpy(emb[own:own + 1]), tmask, SEED_LEN + p, K, 0.1, 0.02, 2.0)
    te = o.text_embeds(r["texts"]).double().numpy()
    te /= np.linalg.norm(te, axis=1, keepdims=True)
    ia = emb.astype(np.float64)
    ia /= np.linalg.norm(ia, axis=1, keepdims=True)
    rv = [int(v) for v in rivals_of_row if v >= 0]
    fin0 = r["final"].double().numpy()[0]
    fin = fin0.copy()
    if rv and delta != 0:
        fin = fin0 + float(delta) * rivals.disc_ref(te @ ia[own], te @ ia[rv].T, scale)
    cand = r["idxs_"].numpy()[0]
    srt = np.sort(fin)[::-1]
    out = (int(cand[int(np.argmax(fin))]), int(cand[int(np.argmax(fin0))]), float(srt[0] - srt[1]))
    _ORACLE_CACHE[key] = out
    return out


@pytest.mark.parametrize("prec", [F32, SPLIT])
def test_teacher_forced_against_the_cpu_oracle(prec):
    """snapshot_every = 1.  For every step and row that runs: the call's ids before the step go through oracle.step.polish_step,
    its texts through o.text_embeds, delta * disc_ref is added in float64, and the winner must be the id the call wrote wherever
    the reference's top-2 margin exceeds 2 * (tol_final(prec) + |delta| * s * 1e-6).  At most a quarter of the row-steps may be
    skipped that way (the oracle chain alone, run on the CPU when the seeds and deltas were chosen, skips none of its 42
    row-steps and its winners with and without the term differ in 34 of them).  The winners with and without the term must
    differ somewhere, on the reference: the test cannot pass with the term ignored."""
    su, emb = _tiny(prec)
    eng = su.engine
    try:
        o = make_oracle(su)
        lens, ior, dl = ORACLE_LENS, ORACLE_IOR, ORACLE_DELTAS
        start, pos, every, hps = _call(su, lens, ior)
        tab = _table(emb, ior)
        ids, _ = eng.generate_rows_vs(start, lens, SEED_LEN, K, pos, hps, None, None, tab, dl, image_of_row=ior, snapshot_every=1)
        scale = float(np.exp(su.clip_cfg.logit_scale))
        n_steps = pos.shape[0]
        assert ids.shape[0] == n_steps
        checked = skipped = moved = 0
        for s in range(n_steps):
            before = start if s == 0 else ids[s - 1]
            for r, n in enumerate(lens):
                p = int(pos[s, r])
                if p == IDLE:
                    np.testing.assert_array_equal(ids[s, r], before[r])
                    continue
                win, win0, margin = oracle_row_step(o, su.token_mask, before[r], n, p, emb, int(ior[r]), tab[r], float(dl[r]), scale)
                moved += int(win != win0)
                if margin <= 2 * (TOL_FINAL[prec] + abs(float(dl[r])) * scale * 1e-6):
                    skipped += 1
                    continue
                checked += 1
                assert int(ids[s, r, SEED_LEN + p]) == win, (prec, s, r, p)
        print(f"[rows_vs] teacher-forced prec {prec}: {checked} row-steps checked, {skipped} skipped as near-ties, "
              f"{moved} where the term moves the reference's winner")
        assert skipped <= (checked + skipped) / 4
        assert moved >= 1
    finally:
        eng.close()


def test_refusals_leave_the_engine_usable():
    su, emb = _tiny(F32)
    eng = su.engine
    try:
        start, pos, every, hps = _call(su)
        tab = _table(emb, IOR)
        good, _ = eng.generate_rows_vs(start, LENS, SEED_LEN, K, pos, hps, None, None, tab, DELTAS, image_of_row=IOR)

        def refused(rv=tab, dl=DELTAS, code=native.ERR_ARG):
            with pytest.raises(native.NativeError) as ei:
                eng.generate_rows_vs(start, LENS, SEED_LEN, K, pos, hps, None, None, rv, dl, image_of_row=IOR)
            assert ei.value.code == code, ei.value
            again, _ = eng.generate_rows_vs(start, LENS, SEED_LEN, K, pos, hps, None, None, tab, DELTAS, image_of_row=IOR)
            np.testing.assert_array_equal(again, good)

        refused(rv=np.full((len(LENS), native.MAX_RIVALS + 1), -1, np.int32))       # M > CZC_MAX_RIVALS
        for bad in (N_IMG, -2):
            t = tab.copy()
            t[2, 0] = bad
            refused(rv=t)                                                            # an index outside [-1, resident batch)
        t = tab.copy()
        t[3, 1] = IOR[3]
        refused(rv=t)                                                                # a rival equal to the row's own image
        t = tab.copy()
        t[4, 0] = -1
        refused(rv=t)                                                                # a filled slot behind an empty one
        for bad in (np.nan, np.inf):
            d = DELTAS.copy()
            d[0] = bad
            refused(dl=d)                                                            # a delta that is not finite
        # M = 0 with an array given: the C ABI directly (the Python method takes M from the table)
        from conzic_amd.engine import hyper_array
        ids = np.empty((2, len(LENS), start.shape[1]), np.int32)
        ln = np.asarray(LENS, np.int32)
        rc = eng.lib.czc_generate_rows_vs(eng.h, len(LENS), start.shape[1], SEED_LEN, start.ctypes.data, ln.ctypes.data, IOR.ctypes.data,
                                          None, K, pos.shape[0], pos.ctypes.data, None, every, hyper_array(hps), None, tab.ctypes.data,
                                          0, DELTAS.ctypes.data, ids.ctypes.data, None)
        assert rc == native.ERR_ARG
        again, _ = eng.generate_rows_vs(start, LENS, SEED_LEN, K, pos, hps, None, None, tab, DELTAS, image_of_row=IOR)
        np.testing.assert_array_equal(again, good)
    finally:
        eng.close()


def test_refine_engine_refuses_and_stays_usable():
    su, emb = _tiny(REFINE)
    eng = su.engine
    try:
        start, pos, every, hps = _call(su)
        tab = _table(emb, IOR)
        with pytest.raises(native.NativeError, match="SPLIT") as ei:
            eng.generate_rows_vs(start, LENS, SEED_LEN, K, pos, hps, None, None, tab, DELTAS, image_of_row=IOR)
        assert ei.value.code == native.ERR_STATE
        ids0, cos0 = eng.generate_rows_tied(start, LENS, SEED_LEN, K, pos, hps, None, None, image_of_row=IOR)
        ids1, cos1 = eng.generate_rows_vs(start, LENS, SEED_LEN, K, pos, hps, None, None, tab, np.zeros(len(LENS), np.float32), image_of_row=IOR)
        np.testing.assert_array_equal(ids0, ids1)
        cos, disc = eng.score_rows_vs(ids0[-1], SEED_LEN, tab, LENS, IOR)       # works on every precision
        np.testing.assert_array_equal(_bits(cos), _bits(eng.score_rows(ids0[-1], SEED_LEN, LENS, IOR)))
        assert ((disc > 0) & (disc < 1)).all()
    finally:
        eng.close()


def _clip_ids(su, rows, lens):
    bpe = T.ClipBpe(su.sv.clip_vocab, su.sv.clip_merges)
    out = [T.bridge([int(t) for t in rows[r, :SEED_LEN + n + 1]], su.sv.bert_tokens, bpe) for r, n in enumerate(lens)]
    ids = np.full((len(out), max(len(o) for o in out)), su.clip_cfg.eos_id, dtype=np.int32)
    for r, o in enumerate(out):
        ids[r, :len(o)] = o
    return ids, np.array([len(o) for o in out], dtype=np.int32)


def _disc64(text, emb, ior, tab, scale):
    t = np.asarray(text, np.float64)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    ia = emb.astype(np.float64)
    ia /= np.linalg.norm(ia, axis=1, keepdims=True)
    c0 = (t * ia[ior]).sum(1)
    cj = np.einsum("rd,rmd->rm", t, ia[np.maximum(tab, 0)])
    return rivals.disc_ref(c0, cj, scale, tab >= 0)


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_score_rows_vs(prec):
    """out_cos has the bits of score_rows; out_disc is the host path's (bridge -> encode_text -> disc_ref) within s * 1e-6; a row
    without rivals has disc = 1; and with no table every disc is 1."""
    su, emb = _tiny(prec)
    eng = su.engine
    try:
        rows = lengths.length_rows(su.bert_tok, PROMPT, LENS)
        regular = np.nonzero(su.token_mask[0] > 0)[0]
        rng = np.random.default_rng(17)
        for r, n in enumerate(LENS):
            rows[r, SEED_LEN:SEED_LEN + n] = rng.choice(regular, size=n)
        tab = _table(emb, IOR)
        tab[4, :] = -1
        tab[6, 1] = -1
        cos, disc = eng.score_rows_vs(rows, SEED_LEN, tab, LENS, IOR)
        np.testing.assert_array_equal(_bits(cos), _bits(eng.score_rows(rows, SEED_LEN, LENS, IOR)))
        cids, clen = _clip_ids(su, rows, LENS)
        scale = float(np.exp(su.clip_cfg.logit_scale))
        want = _disc64(eng.encode_text(cids, clen), emb, IOR, tab, scale)
        err = float(np.abs(disc.astype(np.float64) - want).max())
        print(f"[score_rows_vs] prec {prec}: worst |d disc| against bridge -> encode_text -> disc_ref {err:.3e} (bar {scale * 1e-6:.3e})")
        assert err <= scale * 1e-6
        assert disc[4] == 1.0
        _, ones = eng.score_rows_vs(rows, SEED_LEN, None, LENS, IOR)
        assert (ones == 1.0).all()
    finally:
        eng.close()


def test_score_rows_vs_f32_against_the_cpu_oracle():
    from oracle import models as M
    su, emb = _tiny(F32)
    eng = su.engine
    try:
        rows = lengths.length_rows(su.bert_tok, PROMPT, LENS)
        regular = np.nonzero(su.token_mask[0] > 0)[0]
        rng = np.random.default_rng(18)
        for r, n in enumerate(LENS):
            rows[r, SEED_LEN:SEED_LEN + n] = rng.choice(regular, size=n)
        tab = _table(emb, IOR)
        _, disc = eng.score_rows_vs(rows, SEED_LEN, tab, LENS, IOR)
        cids, clen = _clip_ids(su, rows, LENS)
        w = M.to_torch(synth.make_clip_weights(su.clip_cfg, 12))
        ref = M.clip_text_embeds(w, su.clip_cfg, torch.from_numpy(cids.astype(np.int64)), torch.from_numpy(clen.astype(np.int64)))
        scale = float(np.exp(su.clip_cfg.logit_scale))
        err = float(np.abs(disc.astype(np.float64) - _disc64(ref.double().numpy(), emb, IOR, tab, scale)).max())
        print(f"[score_rows_vs] F32: worst |d disc| against oracle.models.clip_text_embeds {err:.3e} (bar {scale * 1e-5:.3e})")
        assert err <= scale * 1e-5
    finally:
        eng.close()
