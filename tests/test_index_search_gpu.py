"""-m gpu: czc_index_set / czc_index_search (include/conzic_hip.h, csrc/retrieve.hip) against the fp64 reference of
tests/retrieval_ref.py.

Bar: 2e-6 on a cosine against fp64, what the project's fp32-class paths are held to.  Random rows are near-ties at this
precision, so ids are asserted exactly only on planted inputs; everywhere else a returned id must carry its own fp64 cosine
and the j-th returned cosine must be the j-th largest, both within the bar.  Every test prints the worst error it saw."""
import dataclasses

import numpy as np
import pytest

import retrieval_ref as ref
from conzic_amd import harness, native, synth
from conzic_amd.engine import Engine, NativeError

pytestmark = pytest.mark.gpu
BAR = 2e-6
WORST = [0.0]
PLANT_ROWS = (0, 31, 32, 500, 999)
PLANT_COS = (0.95, 0.90, 0.85, 0.80, 0.75)
PLANT_SEED = 20


@pytest.fixture(scope="module")
def eng64():
    su = harness.build_synthetic(True, native.PREC_F32)
    assert su.clip_cfg.proj == 64
    yield su.engine
    su.engine.close()


@pytest.fixture(scope="module")
def eng512():
    sv = harness.cached_vocab(True)
    cfg = dataclasses.replace(synth.clip_tiny(len(sv.clip_vocab)), proj=512)
    su = harness.build_synthetic(True, native.PREC_SPLIT, clip_cfg=cfg)
    yield su.engine
    su.engine.close()


def _note(err, what):
    WORST[0] = max(WORST[0], float(err))
    print(f"index search, {what}: worst |cosine - fp64| {float(err):.3e} (all tests so far {WORST[0]:.3e}, bar {BAR:.0e})")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(ids, cos, q, X, k, what):
    """The shape-independent properties of a result; returns the worst cosine error."""
    sc = ref.scores(q, X)
    Q, N = sc.shape
    m = min(k, N)
    assert ids.shape == (Q, k) and cos.shape == (Q, k) and ids.dtype == np.int32 and cos.dtype == np.float32
    assert (ids[:, m:] == -1).all() and np.isneginf(cos[:, m:]).all(), what
    worst = 0.0
    for i in range(Q):
        got_i, got_c = ids[i, :m], cos[i, :m].astype(np.float64)
        assert np.isfinite(got_c).all(), what
        assert (np.diff(got_c) <= 0).all(), (what, "cosines must be non-increasing")
        assert ((got_i >= 0) & (got_i < N)).all() and np.unique(got_i).size == m, (what, got_i)
        top = np.sort(sc[i])[::-1][:m]
        e1 = np.abs(got_c - top).max()          # the j-th returned cosine is the j-th largest
        e2 = np.abs(got_c - sc[i, got_i]).max()  # and belongs to the id it came with
        assert e1 <= BAR and e2 <= BAR, (what, i, e1, e2)
        worst = max(worst, e1, e2)
    return worst


def _plant(rng, N, D):
    """Three queries of mutual cosine 0.8 and a random crowd of N rows in which rows PLANT_ROWS carry, for query q, the
    cosines PLANT_COS shifted cyclically by q (every query has all five, each at another row).  Returns (queries, rows,
    expected ids [3, 5])."""
    E = np.linalg.qr(rng.standard_normal((D, 3)))[0].T    # orthonormal e0, e1, e2
    ring = [E[1], -0.5 * E[1] + np.sqrt(0.75) * E[2], -0.5 * E[1] - np.sqrt(0.75) * E[2]]
    # mutual cosine 13/15 - (2/15) / 2 = 0.8: three such queries can see (0.95, 0.75, 0.80) on one row, orthogonal ones cannot
    U = np.array([np.sqrt(13 / 15) * E[0] + np.sqrt(2 / 15) * r for r in ring])
    G = U @ U.T
    X = rng.standard_normal((N, D))
    want = np.zeros((3, 5), dtype=np.int32)
    for r, row in enumerate(PLANT_ROWS):
        c = np.array([PLANT_COS[(r - q) % 5] for q in range(3)])
        a = np.linalg.solve(G, c)
        rest = 1.0 - c @ a
        assert rest > 0, (row, rest)
        w = rng.standard_normal(D)
        w -= U.T @ np.linalg.solve(G, U @ w)
        X[row] = U.T @ a + np.sqrt(rest) * w / np.linalg.norm(w)
        for q in range(3):
            want[q, (r - q) % 5] = row
    return U.astype(np.float32), X.astype(np.float32), want


def _assert_planted(q, X, want):
    """On the fp64 reference: neighbouring planted scores more than 1e-3 apart, the crowd below them by more than 1e-2."""
    sc = ref.scores(q, X)
    for i in range(3):
        planted = sc[i, want[i]]
        assert (planted[:-1] - planted[1:] > 1e-3).all(), planted
        crowd = np.delete(sc[i], want[i])
        assert planted[-1] - crowd.max() > 1e-2, (planted[-1], crowd.max())
    return sc


@pytest.mark.parametrize("D", [64, 512])
def test_planted_winners(D, eng64, eng512):
    eng = eng64 if D == 64 else eng512
    q, X, want = _plant(np.random.default_rng(PLANT_SEED), 1000, D)
    sc = _assert_planted(q, X, want)
    eng.index_set(X)
    assert eng.index_size() == 1000
    ids, cos = eng.index_search(q, 5)
    assert (ids == want).all(), (ids, want)
    err = np.abs(cos.astype(np.float64) - np.take_along_axis(sc, want, 1)).max()
    _note(err, f"planted winners D={D}")
    assert err <= BAR


@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("N", [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 4099])
def test_shapes(N, k, eng64):
    rng = np.random.default_rng(1000 * N + k)
    X = rng.standard_normal((N, 64)).astype(np.float32)
    q = rng.standard_normal((3, 64)).astype(np.float32)
    eng64.index_set(X)
    worst, first = 0.0, None
    try:
        for groups in (0, 1, 3, 7):
            eng64.set_option("index_groups", groups)
            ids, cos = eng64.index_search(q, k)
            worst = max(worst, _check(ids, cos, q, X, k, f"N={N} k={k} groups={groups}"))
            if first is None:
                first = (ids, cos)
            assert (ids == first[0]).all() and (_bits(cos) == _bits(first[1])).all(), ("group count changed the result", groups)
    finally:
        eng64.set_option("index_groups", 0)
    _note(worst, f"shapes N={N} k={k}")


@pytest.mark.parametrize("D", [64, 512])
@pytest.mark.parametrize("N", [33, 257])
def test_all_cosines_negative(N, D, eng64, eng512):
    """Queries point away from a clustered index: a slot won by a padding row, by a zero query column or by an initial value
    would carry a cosine of 0 or an id out of range."""
    eng = eng64 if D == 64 else eng512
    rng = np.random.default_rng(7 * N + D)
    centre = rng.standard_normal(D)
    X = (centre + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    q = (-centre + 0.3 * rng.standard_normal((3, D))).astype(np.float32)
    assert ref.scores(q, X).max() < -0.5
    eng.index_set(X)
    worst = 0.0
    for k in (5, 64):
        for groups in (0, 3):
            eng.set_option("index_groups", groups)
            ids, cos = eng.index_search(q, k)
            eng.set_option("index_groups", 0)
            worst = max(worst, _check(ids, cos, q, X, k, f"negative N={N} D={D} k={k} groups={groups}"))
            assert (cos[:, :min(k, N)] < -0.5).all()
    _note(worst, f"all cosines negative N={N} D={D}")


@pytest.mark.parametrize("Q", [1, 2, 31, 32, 33, 65])
def test_query_tiles(Q, eng64):
    """Row q of a batched call = the call with that query alone, bit for bit."""
    rng = np.random.default_rng(50 + Q)
    X = rng.standard_normal((1000, 64)).astype(np.float32)
    q = rng.standard_normal((Q, 64)).astype(np.float32)
    eng64.index_set(X)
    ids, cos = eng64.index_search(q, 5)
    _note(_check(ids, cos, q, X, 5, f"Q={Q}"), f"query tiles Q={Q}")
    for i in range(Q):
        i1, c1 = eng64.index_search(q[i:i + 1], 5)
        assert (i1[0] == ids[i]).all() and (_bits(c1[0]) == _bits(cos[i])).all(), i


def test_placement_permuted_index(eng64):
    """The cosine of a (query, row) pair has the same bits wherever the row sits."""
    rng = np.random.default_rng(77)
    q = rng.standard_normal((3, 64)).astype(np.float32)
    for N in (64, 1000):  # 64: k = 64 returns every row; 1000: the 64 best of 32 blocks
        X = rng.standard_normal((N, 64)).astype(np.float32)
        perm = rng.permutation(N)
        eng64.index_set(X)
        ids_a, cos_a = eng64.index_search(q, 64)
        eng64.index_set(X[perm])          # new row j is original row perm[j]
        ids_b, cos_b = eng64.index_search(q, 64)
        for i in range(3):
            a = dict(zip(ids_a[i].tolist(), _bits(cos_a[i]).tolist()))
            b = dict(zip(perm[ids_b[i]].tolist(), _bits(cos_b[i]).tolist()))
            assert len(a) == 64 and a == b, (N, i)


@pytest.mark.parametrize("D", [64, 512])
def test_placement_group_counts(D, eng64, eng512):
    eng = eng64 if D == 64 else eng512
    rng = np.random.default_rng(78 + D)
    X = rng.standard_normal((4099, D)).astype(np.float32)
    q = rng.standard_normal((5, D)).astype(np.float32)
    eng.index_set(X)
    out = []
    try:
        for groups in (1, 3, 7, 0):
            eng.set_option("index_groups", groups)
            assert eng.get_option("index_groups") == groups
            out.append(eng.index_search(q, 64))
    finally:
        eng.set_option("index_groups", 0)
    _note(_check(out[0][0], out[0][1], q, X, 64, f"groups D={D}"), f"group counts D={D}")
    for ids, cos in out[1:]:
        assert (ids == out[0][0]).all() and (_bits(cos) == _bits(out[0][1])).all()


def test_duplicates_come_back_lowest_id_first(eng64):
    rng = np.random.default_rng(91)
    q, X, want = _plant(rng, 1000, 64)
    _assert_planted(q, X, want)
    copies = [3, 31, 32, 100, 257, 500, 777, 998, 999]
    X[copies] = X[0]          # query 0's best row (cosine 0.95): ten of it with row 0, over the blocks and groups
    eng64.index_set(X)
    try:
        for groups in (0, 1, 3, 7):
            eng64.set_option("index_groups", groups)
            ids, cos = eng64.index_search(q[:1], 5)
            assert ids[0].tolist() == [0, 3, 31, 32, 100], (groups, ids)
            assert (_bits(cos[0]) == _bits(cos[0])[0]).all(), (groups, cos)
            assert abs(float(cos[0, 0]) - ref.scores(q[:1], X)[0, 0]) <= BAR
    finally:
        eng64.set_option("index_groups", 0)


def test_normalisation(eng64):
    """Rows and queries scaled by 1e-3 ... 1e3 give the ids of the unit-norm call and cosines within the bar."""
    rng = np.random.default_rng(PLANT_SEED)
    q, X, want = _plant(rng, 1000, 64)
    eng64.index_set(X)
    ids0, _ = eng64.index_search(q, 5)
    Xs = (X * 10.0 ** rng.uniform(-3, 3, size=(1000, 1))).astype(np.float32)
    qs = (q * np.array([[1e-3], [1.0], [1e3]])).astype(np.float32)
    sc = _assert_planted(qs, Xs, want)
    eng64.index_set(Xs)
    ids, cos = eng64.index_search(qs, 5)
    assert (ids == ids0).all() and (ids == want).all()
    err = np.abs(cos.astype(np.float64) - np.take_along_axis(sc, want, 1)).max()
    _note(err, "scaled rows and queries")
    assert err <= BAR


def test_errors(eng64):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((100, 64)).astype(np.float32)
    q = rng.standard_normal((3, 64)).astype(np.float32)
    eng64.index_clear()
    assert eng64.index_size() == 0
    with pytest.raises(NativeError) as ei:
        eng64.index_search(q, 5)
    assert ei.value.code == native.ERR_STATE
    eng64.index_set(X)
    before = eng64.index_search(q, 5)
    for poison in (0.0, np.nan, np.inf):
        bad = rng.standard_normal((300, 64)).astype(np.float32)
        bad[257] = poison
        with pytest.raises(NativeError) as ei:
            eng64.index_set(bad)
        assert ei.value.code == native.ERR_ARG
        assert eng64.index_size() == 100          # the old index still answers
        after = eng64.index_search(q, 5)
        assert (after[0] == before[0]).all() and (_bits(after[1]) == _bits(before[1])).all()
    for poison in (0.0, np.nan):
        qb = q.copy()
        qb[1] = poison
        with pytest.raises(NativeError) as ei:
            eng64.index_search(qb, 5)
        assert ei.value.code == native.ERR_ARG
    for k in (0, 65):
        with pytest.raises(NativeError) as ei:
            eng64.index_search(q, k)
        assert ei.value.code == native.ERR_ARG
    ids, cos = eng64.index_search(q, native.INDEX_MAX_K)
    assert ids.shape == (3, 64)
    for groups in (-1, 1025):
        with pytest.raises(NativeError) as ei:
            eng64.set_option("index_groups", groups)
        assert ei.value.code == native.ERR_ARG
    # image_embeds = NULL: the engine's resident image embeddings
    eng64.set_image_embeds(q)
    r_ids, r_cos = eng64.index_search(None, 5, Q=3)
    assert (r_ids == before[0]).all() and (_bits(r_cos) == _bits(before[1])).all()
    with pytest.raises(NativeError) as ei:
        eng64.index_search(None, 5, Q=4)          # more than are resident
    assert ei.value.code == native.ERR_ARG


def test_replace_and_drop(eng64):
    rng = np.random.default_rng(6)
    q = rng.standard_normal((3, 64)).astype(np.float32)
    eng64.index_set(rng.standard_normal((1000, 64)).astype(np.float32))
    assert eng64.index_size() == 1000
    X = rng.standard_normal((10, 64)).astype(np.float32)
    eng64.index_set(X)
    assert eng64.index_size() == 10
    ids, cos = eng64.index_search(q, 64)
    assert ids.max() < 10
    _note(_check(ids, cos, q, X, 64, "replaced index"), "replaced index")
    rep = eng64.replica()
    assert rep.index_size() == 0                  # a replica has no index
    with pytest.raises(NativeError) as ei:
        rep.index_search(q, 1)
    assert ei.value.code == native.ERR_STATE
    eng64.index_clear()
    assert eng64.index_size() == 0
    with pytest.raises(NativeError) as ei:
        eng64.index_search(q, 1)
    assert ei.value.code == native.ERR_STATE


def test_engine_state_is_untouched():
    """A short czc_generate returns the same ids and cosines before an index set-and-search and after it."""
    su = harness.build_synthetic(True, native.PREC_SPLIT)
    eng = su.engine
    try:
        rng = np.random.default_rng(3)
        B, L = 2, 4
        emb = rng.standard_normal((B, su.clip_cfg.proj)).astype(np.float32)
        init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)

        def run():
            eng.set_image_embeds(emb)
            return eng.generate(B, init, L, 4, 8, list(range(L)) * 2, Engine.hyper(0.02, 2.0, 0.1))

        ids0, cos0 = run()
        X = rng.standard_normal((4099, su.clip_cfg.proj)).astype(np.float32)
        eng.index_set(X)
        s_ids, s_cos = eng.index_search(None, 5, Q=B)
        _check(s_ids, s_cos, emb, X, 5, "resident embeddings")
        ids1, cos1 = run()
        assert (np.asarray(ids0) == np.asarray(ids1)).all()
        assert (_bits(np.asarray(cos0)) == _bits(np.asarray(cos1))).all()
    finally:
        eng.close()
