"""czc_fluency_rows end to end (tiny synthetic towers unless noted): against the float64 oracle of tests/fluency_ref.py, against the
step's own logits and candidate list, across chunk sizes, row orders and companions, its refusals and the state it leaves.

Bars.  The project's logit bars (test_step_gpu.py test_bert_logits_row_vs_reference): 5e-5 on F32, 2e-4 on the split-fp16 BERT tower
(the BF16 and SPLIT engines).  Since |d(x_t - lse)| <= 2 max|dx|, a log-probability may differ by 2 x logit bar / t, a row's PLL by
L_r times that.  Ranks are compared wherever the oracle's logit gap to both rank neighbours exceeds twice the logit bar."""
import numpy as np
import pytest

import fluency_ref as FR
from conzic_amd import harness, native, synth
from conzic_amd.engine import Engine

pytestmark = pytest.mark.gpu

F32, SPLIT, BF16 = native.PREC_F32, native.PREC_SPLIT, native.PREC_BF16
SEED_LEN = FR.E2E_SEED_LEN


def _logit_bar(prec):
    return FR.LOGIT_BAR["f32" if prec == F32 else "split"]


@pytest.fixture(scope="module")
def setups():
    made = {}

    def get(prec):
        if prec not in made:
            made[prec] = harness.build_synthetic(True, prec)
        return made[prec]
    yield get
    for su in made.values():
        su.engine.close()


_oracle_cache = {}


def _case(su, dense, temperature, prec):
    """rows, lens and the oracle's (logp, rank, sure) of one end-to-end case; computed once per (dense, t, bar)."""
    sp = harness.special_ids(su.bert_tok)
    regular = np.nonzero(synth.make_token_mask(su.sv)[0] > 0)[0]
    rows, lens = FR.e2e_rows(sp, regular, dense)
    key = (dense, temperature, _logit_bar(prec))
    if key not in _oracle_cache:
        _oracle_cache[key] = FR.oracle_fluency(synth.make_bert_weights(su.bert_cfg, 11), su.bert_cfg, rows, SEED_LEN, lens, sp["[MASK]"],
                                               temperature, _logit_bar(prec))[:3]
    return rows, lens, _oracle_cache[key]


def _check_against(res, lens, ref, bar, what):
    """logp within `bar` per position, pll within L_r x bar, rank equal wherever the oracle is sure (at most 2 % left out), padding."""
    logp, rank, sure = ref
    worst = 0.0
    n, n_sure = sum(lens), 0
    for r, L in enumerate(lens):
        err = np.abs(res["logp"][r, :L].astype(np.float64) - logp[r, :L])
        worst = max(worst, float(err.max()))
        assert err.max() <= bar, (what, r, err)
        assert abs(float(res["pll"][r]) - logp[r, :L].sum()) <= L * bar, (what, r)
        assert (res["logp"][r, L:] == 0.0).all() and (res["rank"][r, L:] == -1).all(), (what, r)
        ok = sure[r, :L]
        n_sure += int(ok.sum())
        assert (res["rank"][r, :L][ok] == rank[r, :L][ok]).all(), (what, r, res["rank"][r, :L], rank[r, :L])
    assert n - n_sure <= 0.02 * n, (what, n, n_sure)
    return worst


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("prec", [F32, SPLIT, BF16])
def test_against_the_cpu_oracle(setups, prec, dense):
    su = setups(prec)
    for t in (1.0, 0.5):
        rows, lens, ref = _case(su, dense, t, prec)
        res = su.engine.fluency_rows(rows, SEED_LEN, lens=None if dense else lens, temperature=t)
        worst = _check_against(res, lens, ref, 2 * _logit_bar(prec) / t, (prec, dense, t))
        print(f"fluency_rows precision={prec} {'dense' if dense else 'ragged'} t={t}: worst |logp - oracle| = {worst:.2e} "
              f"(bar {2 * _logit_bar(prec) / t:.1e})")
    if dense:   # lens given but all equal: the dense path too, the same bits
        again = su.engine.fluency_rows(rows, SEED_LEN, lens=lens, temperature=0.5)
        np.testing.assert_array_equal(again["logp"], res["logp"])


def test_consistent_with_the_step(setups):
    """On F32 a step on the row's own T_r tokens under an all-ones token mask: its sorted candidate list holds the target at
    `rank`, and the host log-softmax of its logits agrees with logp."""
    su = setups(F32)
    eng, K, t = su.engine, 64, 0.5
    rows, lens, (_, _, sure) = _case(su, False, t, F32)
    res = eng.fluency_rows(rows, SEED_LEN, lens=lens, temperature=t)
    V = su.bert_cfg.vocab
    try:
        eng.set_token_mask(np.ones((1, V), dtype=np.float32))
        eng.set_image_embeds(np.random.default_rng(1).standard_normal((1, su.clip_cfg.proj)).astype(np.float32))
        hp = Engine.hyper(0.02, 2.0, t)
        bar, checked = 2 * _logit_bar(F32) / t, 0
        for r, L in enumerate(lens):
            for j in range(L):
                inp = np.ascontiguousarray(rows[r:r + 1, :SEED_LEN + L + 1])
                target = int(inp[0, SEED_LEN + j])
                out = eng.step(inp.copy(), SEED_LEN + j, K, hp, dot_allowed=True, want=("logits", "idxs"))
                y = out["logits"][0].astype(np.float64) / t
                lse = y.max() + np.log(np.exp(y - y.max()).sum())
                assert abs((y[target] - lse) - float(res["logp"][r, j])) <= bar, (r, j)
                rk = int(res["rank"][r, j])
                if rk < K and sure[r, j]:
                    assert int(out["idxs"][0, rk]) == target, (r, j, rk)
                    checked += 1
        assert checked >= 1
    finally:
        eng.set_token_mask(su.token_mask)


def test_chunks_row_orders_and_companions(setups):
    su = setups(SPLIT)
    eng, t = su.engine, 1.0
    rows, lens, _ = _case(su, False, t, SPLIT)
    bar = 2 * _logit_bar(SPLIT) / t
    base = eng.fluency_rows(rows, SEED_LEN, lens=lens, temperature=t)
    twice = eng.fluency_rows(rows, SEED_LEN, lens=lens, temperature=t)
    for k in ("logp", "rank", "pll"):
        np.testing.assert_array_equal(base[k], twice[k])     # the same call: the same bits

    def close(res, idx, what):
        for i, r in enumerate(idx):
            L = lens[r]
            assert np.abs(res["logp"][i, :L] - base["logp"][r, :L]).max() <= bar, (what, r)
            assert abs(float(res["pll"][i]) - float(base["pll"][r])) <= L * bar, (what, r)
            assert (res["logp"][i, L:] == 0).all() and (res["rank"][i, L:] == -1).all(), (what, r)
    try:
        for chunk in (1, 7, 1024):
            eng.set_option("fluency_chunk", chunk)
            assert eng.get_option("fluency_chunk") == chunk
            close(eng.fluency_rows(rows, SEED_LEN, lens=lens, temperature=t), range(len(lens)), f"chunk {chunk}")
    finally:
        eng.set_option("fluency_chunk", 1024)
    perm = [3, 0, 4, 2, 1]
    close(eng.fluency_rows(rows[perm], SEED_LEN, lens=[lens[r] for r in perm], temperature=t), perm, "permuted")
    for r in (0, 2):
        close(eng.fluency_rows(rows[r:r + 1], SEED_LEN, lens=[lens[r]], temperature=t), [r], "alone")
    # a torch tensor on the device is scored where it lies
    import torch
    dev = eng.fluency_rows(torch.from_numpy(rows).to("cuda"), SEED_LEN, lens=lens, temperature=t)
    np.testing.assert_array_equal(dev["logp"], base["logp"])
    # any output may be NULL, not all three
    lib, R, T = eng.lib, rows.shape[0], rows.shape[1]
    pll = np.empty((R,), np.float32)
    ln = np.asarray(lens, dtype=np.int32)
    assert lib.czc_fluency_rows(eng.h, rows.ctypes.data, R, T, SEED_LEN, ln.ctypes.data, t, None, None, pll.ctypes.data) == 0
    np.testing.assert_array_equal(pll, base["pll"])


def test_refusals_leave_the_engine_usable(setups):
    su = setups(SPLIT)
    eng = su.engine
    rows, lens, _ = _case(su, False, 1.0, SPLIT)
    good = eng.fluency_rows(rows, SEED_LEN, lens=lens)
    R, T = rows.shape
    V = su.bert_cfg.vocab
    lib = eng.lib
    out = np.empty((R, T), np.float32)

    def call(rows_=rows, R_=R, T_=T, seed_len=SEED_LEN, lens_=lens, t=1.0, outs=True):
        ln = None if lens_ is None else np.asarray(lens_, dtype=np.int32)
        r = np.ascontiguousarray(rows_, dtype=np.int32)
        return lib.czc_fluency_rows(eng.h, r.ctypes.data, R_, T_, seed_len, None if ln is None else ln.ctypes.data, t,
                                    out.ctypes.data if outs else None, None, None)
    bad_id, bad_tail = rows.copy(), rows.copy()
    bad_id[1, SEED_LEN] = V
    bad_tail[0, T - 1] = -5            # behind row 0's own tokens: not read, not refused
    big = np.zeros((1, native.MAX_BERT_LEN + 1), np.int32)
    cases = {
        "R = 0": call(R_=0), "R too large": call(R_=16385), "T = 0": call(T_=0), "T too large": call(rows_=big, R_=1, T_=big.shape[1], lens_=None),
        "seed_len < 0": call(seed_len=-1), "no word": call(seed_len=T - 1, lens_=None), "length 0": call(lens_=[0, 3, 6, 6, 4]),
        "length too large": call(lens_=[1, 3, 7, 6, 4]), "id outside": call(rows_=bad_id), "negative id": call(rows_=-rows),
        "t = 0": call(t=0.0), "t < 0": call(t=-1.0), "t nan": call(t=float("nan")), "t inf": call(t=float("inf")),
        "no output": call(outs=False),
    }
    for what, rc in cases.items():
        assert rc == native.ERR_ARG, (what, rc)
    assert call(rows_=bad_tail) == 0
    with pytest.raises(native.NativeError) as ei:
        eng.set_option("fluency_chunk", 0)
    assert ei.value.code == native.ERR_ARG
    with pytest.raises(native.NativeError):
        eng.set_option("fluency_chunk", 16385)
    fresh = Engine(su.bert_cfg, su.clip_cfg, harness.special_ids(su.bert_tok), SPLIT, 0)   # no weights yet
    try:
        with pytest.raises(native.NativeError) as ei:
            fresh.fluency_rows(rows, SEED_LEN, lens=lens)
        assert ei.value.code == native.ERR_STATE
    finally:
        fresh.close()
    after = eng.fluency_rows(rows, SEED_LEN, lens=lens)
    for k in ("logp", "rank", "pll"):
        np.testing.assert_array_equal(after[k], good[k])


def test_state_the_call_leaves(setups):
    su = setups(SPLIT)
    eng = su.engine
    rows, lens, _ = _case(su, False, 1.0, SPLIT)
    B, L, K = 3, 5, 32
    emb = np.random.default_rng(2).standard_normal((B, su.clip_cfg.proj)).astype(np.float32)
    eng.set_image_embeds(emb)
    init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)
    hp = Engine.hyper(0.02, 2.0, 0.1)
    pos, nm, every = harness.order_positions("sequential", L, 2)
    pos_rows = np.repeat(np.array(pos, dtype=np.int32)[:, None], B, axis=1)
    ids0, cos0 = eng.generate_rows(init, L, SEED_LEN, K, pos_rows, hp, n_mask=nm, snapshot_every=every)
    stats0, opts0 = eng.stats(), {k: eng.get_option(k) for k in ("bert_prune", "memo", "memo_rows", "fluency_chunk")}
    # a step leaves a forward an n_mask = 0 step of the same shape could re-use ...
    inp = np.ascontiguousarray(ids0[-1], dtype=np.int32)
    eng.step(inp.copy(), SEED_LEN + 1, K, hp, n_mask=2)
    eng.step(inp.copy(), SEED_LEN + 2, K, hp, n_mask=0)
    eng.step(inp.copy(), SEED_LEN + 1, K, hp, n_mask=2)
    stats1 = eng.stats()
    eng.fluency_rows(rows, SEED_LEN, lens=lens)
    # ... and the fluency call ends it
    with pytest.raises(native.NativeError, match="n_mask=0") as ei:
        eng.step(inp.copy(), SEED_LEN + 2, K, hp, n_mask=0)
    assert ei.value.code == native.ERR_STATE
    assert eng.stats() == stats1 and stats1 != stats0          # the counters of the generate calls are not the call's
    assert {k: eng.get_option(k) for k in opts0} == opts0
    ids1, cos1 = eng.generate_rows(init, L, SEED_LEN, K, pos_rows, hp, n_mask=nm, snapshot_every=every)   # resident embeds untouched
    np.testing.assert_array_equal(ids1, ids0)
    np.testing.assert_array_equal(cos1, cos0)
    # with the pruned last layer off the call takes the gather path of the MLM head: the same numbers within the bar
    base = eng.fluency_rows(rows, SEED_LEN, lens=lens)
    try:
        eng.set_option("bert_prune", 0)
        full = eng.fluency_rows(rows, SEED_LEN, lens=lens)
    finally:
        eng.set_option("bert_prune", 1)
    for r, Lr in enumerate(lens):
        assert np.abs(full["logp"][r, :Lr] - base["logp"][r, :Lr]).max() <= 2 * _logit_bar(SPLIT)
    with pytest.raises(native.NativeError, match="n_mask=0"):
        eng.step(inp.copy(), SEED_LEN + 2, K, hp, n_mask=0)


def test_full_size_bert_on_split():
    """The one full-size case: bert-base shapes, V = 30 522, R = 2, L = 4, split-fp16 tower, the same bars."""
    su = harness.build_synthetic(False, SPLIT, regular_only=True)
    try:
        sp = harness.special_ids(su.bert_tok)
        rows = np.array(FR.FULL_ROWS, dtype=np.int32)
        lens = [FR.FULL_L] * len(rows)
        assert rows[0, 0] == sp["[CLS]"] and rows[0, -1] == sp["[SEP]"] and su.bert_cfg.vocab == 30522
        for t in (1.0, 0.5):
            ref = FR.oracle_fluency(synth.make_bert_weights(su.bert_cfg, 11), su.bert_cfg, rows, FR.FULL_SEED_LEN, lens, sp["[MASK]"], t,
                                    _logit_bar(SPLIT))[:3]
            res = su.engine.fluency_rows(rows, FR.FULL_SEED_LEN, temperature=t)
            worst = _check_against(res, lens, ref, 2 * _logit_bar(SPLIT) / t, ("full", t))
            print(f"fluency_rows full-size split t={t}: worst |logp - oracle| = {worst:.2e}, ranks {res['rank'].tolist()}")
    finally:
        su.engine.close()
