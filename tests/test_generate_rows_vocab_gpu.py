"""-m gpu: czc_generate_rows_vocab (include/conzic_hip.h) -- a vocabulary set per row of a rows call.  The call is defined by
equivalence (property E of the header): a call whose rows all carry set s returns, bit for bit, what the same call without sets
returns after czc_set_token_mask(token_mask * bits_s); in a mixed call a row returns what the uniform call of its own set returns
for it.  So the yardstick is czc_generate_rows_vs on the same rows under a token mask multiplied on the host, and no tolerance is
needed except where rows run in another packing (ragged lengths and idle steps: the 1e-6 of czc_generate_rows_len on cosines).

Tiny synthetic towers, R = 6 rows over three resident images, L = 5, K = 8, two sweeps of shuffle orders.  Set 0 bans a third of
the regular vocabulary, set 1 allows 120 regular ids."""
import ctypes as C
import random

import numpy as np
import pytest

from conzic_amd import draws as D, harness, lengths, native, rivals, vocab
from conzic_amd.engine import Engine, EngineGroup, _ptr, hyper_array
from conzic_amd.native import NativeError

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT, REFINE = native.PREC_F32, native.PREC_BF16, native.PREC_SPLIT, native.PREC_REFINE
PRECS = [F32, SPLIT, BF16, REFINE]
IDLE = native.POS_IDLE
R, L, K = 6, 5, 8
PROMPT = "Image of a"
SEED_LEN = 4
N_IMG = 3
IOR = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
MIXED = np.array([-1, 0, 1, 0, 1, -1], dtype=np.int32)
TEMPS = [0.1, 0.3, 0.1, 1.0, 0.3, 0.1]


def HP(t=0.1):
    return Engine.hyper(0.02, 2.0, t)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(a, b, what=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what)
    np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]), err_msg=what)


class Setup:
    def __init__(self, prec):
        self.prec = prec
        self.su = harness.build_synthetic(True, prec)
        self.eng = self.su.engine
        self.emb = np.random.default_rng(3).standard_normal((N_IMG, self.su.clip_cfg.proj)).astype(np.float32)
        self.eng.set_image_embeds(self.emb)
        self.mask = self.su.token_mask.reshape(-1).astype(np.float32)
        self.V = self.mask.size
        rng = np.random.default_rng(5)
        regular = np.nonzero(self.mask > 0)[0]
        banned = rng.choice(regular, size=regular.size // 3, replace=False)
        allow0 = np.ones(self.V, bool)
        allow0[banned] = False
        allow1 = np.zeros(self.V, bool)
        allow1[rng.choice(regular, size=120, replace=False)] = True
        self.allowed = np.stack([allow0, allow1])
        self.sets = vocab.pack(list(self.allowed), self.V)
        self.start = lengths.length_rows(self.su.bert_tok, PROMPT, [L] * R)
        self.pos, _, every = lengths.length_schedules([L] * R, "shuffle", 2, rng=random.Random(1))
        assert every == L and (self.pos != IDLE).all() and self.start.shape == (R, SEED_LEN + L + 1)
        self._refs = {}

    def vs(self, hps, draws=None, groups=None, rv=None, dl=None, pos=None, ior=IOR):
        return self.eng.generate_rows_vs(self.start, None, SEED_LEN, K, self.pos if pos is None else pos, hps, draws, groups, rv, dl,
                                         image_of_row=ior)

    def vocab(self, hps, set_of_row, draws=None, groups=None, rv=None, dl=None, pos=None, sets="own", eng=None):
        return (eng or self.eng).generate_rows_vocab(self.start, None, SEED_LEN, K, self.pos if pos is None else pos, hps, draws, groups,
                                                     rv, dl, sets=self.sets if isinstance(sets, str) else sets, set_of_row=set_of_row,
                                                     image_of_row=IOR)

    def premultiplied(self, s, hps, **kw):
        """generate_rows_vs under token_mask * bits_s (s = -1: the mask as it is); the mask is restored"""
        try:
            if s >= 0:
                self.eng.set_token_mask((self.mask * self.allowed[s]).astype(np.float32))
            return self.vs(hps, **kw)
        finally:
            self.eng.set_token_mask(self.mask)

    def ref(self, s, temps):
        """the premultiplied call of set s with a temperature per row, computed once"""
        key = (s, tuple(temps))
        if key not in self._refs:
            self._refs[key] = self.premultiplied(s, [HP(t) for t in temps])
        return self._refs[key]


_setups = {}


@pytest.fixture(scope="module")
def setups():
    def get(prec):
        if prec not in _setups:
            _setups[prec] = Setup(prec)
        st = _setups[prec]
        st.eng.set_option("memo_rows", 0)
        return st
    yield get
    for st in _setups.values():
        st.eng.close()
    _setups.clear()


@pytest.mark.parametrize("prec", PRECS)
def test_uniform_sets_are_the_premultiplied_token_mask(setups, prec):
    """E itself, with equal hyper-parameters in every row (the top-K kernel then reads the records the call filled in) and with
    a temperature per row."""
    st = setups(prec)
    for temps in ([0.1] * R, TEMPS):
        hps = [HP(t) for t in temps]
        for s in (0, 1):
            got = st.vocab(hps, [s] * R)
            _same(got, st.ref(s, temps), f"set {s} temps {temps}")
        assert (st.ref(0, temps)[0] != st.ref(-1, temps)[0]).any() and (st.ref(1, temps)[0] != st.ref(-1, temps)[0]).any()


@pytest.mark.parametrize("prec", PRECS)
def test_mixed_sets_row_by_row(setups, prec):
    st = setups(prec)
    hps = [HP(t) for t in TEMPS]
    ids, cos = st.vocab(hps, MIXED)
    for s in (-1, 0, 1):
        rows = np.nonzero(MIXED == s)[0]
        uni = st.vocab(hps, [s] * R)
        d = float(np.abs(cos[:, rows] - uni[1][:, rows]).max())
        print(f"[rows_vocab] mixed prec {prec} set {s} rows {rows.tolist()}: max |d cos| {d:.3e}, "
              f"{int((ids[:, rows] != uni[0][:, rows]).sum())} ids differ")
        _same((ids[:, rows], cos[:, rows]), (uni[0][:, rows], uni[1][:, rows]), f"set {s}")
        _same((ids[:, rows], cos[:, rows]), (st.ref(s, TEMPS)[0][:, rows], st.ref(s, TEMPS)[1][:, rows]), f"set {s} (premultiplied)")


@pytest.mark.parametrize("prec", PRECS)
def test_null_and_all_minus_one_are_generate_rows_vs(setups, prec):
    st = setups(prec)
    hps = [HP(t) for t in TEMPS]
    want = st.ref(-1, TEMPS)
    _same(st.vocab(hps, None), want, "set_of_row = None")
    _same(st.vocab(hps, None, sets=None), want, "sets = None, set_of_row = None")
    _same(st.vocab(hps, [-1] * R), want, "all -1")


@pytest.mark.parametrize("prec", PRECS)
def test_the_restriction_bites(setups, prec):
    """Every row is banned the words its unconstrained run ended with ('.' and [PAD] aside: the '.' rule overrides a set, and
    [PAD] is what a removed id turns into): none of them comes back, and the captions change."""
    st = setups(prec)
    hps = [HP() for _ in range(R)]
    free = st.ref(-1, [0.1] * R)[0][-1]
    dot, pad = int(st.su.bert_tok.vocab["."]), int(st.su.bert_tok.pad_token_id)
    ended = [sorted(set(int(i) for i in free[r, SEED_LEN:SEED_LEN + L]) - {dot, pad}) for r in range(R)]
    assert all(ended)
    masks = np.ones((R, st.V), bool)
    for r in range(R):
        masks[r, ended[r]] = False
    ids, _ = st.vocab(hps, np.arange(R), sets=vocab.pack(list(masks), st.V))
    for snap in ids:
        for r in range(R):
            assert not set(int(i) for i in snap[r, SEED_LEN:SEED_LEN + L]) & set(ended[r]), (r, snap[r])
    assert (ids[-1] != free).any(axis=1).sum() >= 1


@pytest.mark.parametrize("prec", PRECS)
def test_memo_rows_on_equals_off(setups, prec):
    st = setups(prec)
    hps = [HP(t) for t in TEMPS]
    pos = np.tile(st.pos[:L], (4, 1))   # four sweeps of the same orders: settled rows hit
    off = st.vocab(hps, MIXED, pos=pos)
    try:
        st.eng.set_option("memo_rows", 1)
        on = st.vocab(hps, MIXED, pos=pos)
        stats = st.eng.memo_rows_stats()
    finally:
        st.eng.set_option("memo_rows", 0)
    print(f"[rows_vocab] memo_rows prec {prec}: {stats}")
    _same(on, off)


@pytest.mark.parametrize("prec", PRECS)
def test_idle_steps_and_ragged_lengths(setups, prec):
    """Rows of lengths 3, 5, 4, 5, 1, 5 in one call (shorter rows sit out the tail of a sweep): every row returns what a call of
    that row alone, at its own length and without idle steps, returns -- ids exactly, cosines within 1e-6 (the bar
    czc_generate_rows_len states for rows that run in another packing).

    Measured on the MI355X: F32 and BF16 0 everywhere, SPLIT at most 7.5e-8, CZC_PREC_REFINE at most 6.0e-8; ids identical on
    all four.  On CZC_PREC_REFINE this rests on the step rule of run_steps: a row that is idle at a snapshot step returns the
    cosine of its last step, so that step re-encodes a gated row's winner as a snapshot step does (before that rule such a row
    returned its screening cosine, 1.06e-4 away)."""
    st = setups(prec)
    lens = [3, 5, 4, 5, 1, 5]
    start = lengths.length_rows(st.su.bert_tok, PROMPT, lens)
    pos, n_mask, every = lengths.length_schedules(lens, "shuffle", 2, rng=random.Random(4))
    assert (pos == IDLE).any()
    hps = [HP(t) for t in TEMPS]
    ids, cos = st.eng.generate_rows_vocab(start, lens, SEED_LEN, K, pos, hps, sets=st.sets, set_of_row=MIXED, image_of_row=IOR,
                                          n_mask=n_mask)
    for r, n in enumerate(lens):
        T_r = SEED_LEN + n + 1
        pos_r = np.ascontiguousarray(pos[:, r:r + 1].reshape(2, every)[:, :n].reshape(-1, 1))
        assert (pos_r != IDLE).all()
        one = st.eng.generate_rows_vocab(start[r:r + 1, :T_r], [n], SEED_LEN, K, pos_r, [hps[r]], sets=st.sets, set_of_row=MIXED[r:r + 1],
                                         image_of_row=IOR[r:r + 1])
        d = float(np.abs(cos[:, r] - one[1][:, 0]).max())
        print(f"[rows_vocab] ragged prec {prec} row {r} len {n}: max |d cos| {d:.3e}")
        np.testing.assert_array_equal(ids[:, r, :T_r], one[0][:, 0])
        assert (ids[:, r, T_r:] == 0).all()
        np.testing.assert_allclose(cos[:, r], one[1][:, 0], rtol=0, atol=1e-6)


@pytest.mark.parametrize("prec", [F32, BF16])
def test_groups_draws_and_rivals_ride_with_sets(setups, prec):
    """Tied groups, draws with tau > 0 and rivals with delta != 0 in the same call: E still holds."""
    st = setups(prec)
    hps = [HP(t) for t in TEMPS]
    draws = D.draw_rows([D.row_seed(7, 0, i) for i in range(R)], [0.5, 0.0, 0.3, 0.5, 0.0, 0.3])
    tab = rivals.expand(rivals.rival_table(st.emb, 2), IOR)
    dl = np.array([1.0, 0.5, 2.0, 1.0, 0.0, 0.5], np.float32)
    # draws and rivals with the rows' own orders
    for s in (0, 1):
        got = st.vocab(hps, [s] * R, draws=draws, rv=tab, dl=dl)
        _same(got, st.premultiplied(s, hps, draws=draws, rv=tab, dl=dl), f"draws + rivals, set {s}")
    # tied groups of two rows (one image, one start row, neighbouring positions of one order), with draws and rivals
    groups = np.array([0, 0, 1, 1, 2, 2], np.int32)
    ior = np.array([0, 0, 1, 1, 2, 2], np.int32)
    tab_g = rivals.expand(rivals.rival_table(st.emb, 2), ior)
    pos = st.pos.copy()
    pos[:, 1::2] = (pos[:, 0::2] + 1) % L
    kw = dict(draws=draws, groups=groups, rv=tab_g, dl=dl, pos=pos)
    for s in (0, 1):
        got = st.eng.generate_rows_vocab(st.start, None, SEED_LEN, K, pos, hps, draws, groups, tab_g, dl, sets=st.sets, set_of_row=[s] * R,
                                         image_of_row=ior)
        _same(got, st.premultiplied(s, hps, ior=ior, **kw), f"groups + draws + rivals, set {s}")


@pytest.mark.parametrize("prec", [F32, BF16])
def test_engine_group_over_two_streams(setups, prec):
    st = setups(prec)
    hps = [HP(t) for t in TEMPS]
    want = st.vocab(hps, MIXED)
    grp = EngineGroup(st.eng, streams=2, min_images=1)
    try:
        grp.set_image_embeds(st.emb)
        assert len(grp.parts(R)) == 2
        got = grp.generate_rows_vocab(st.start, None, SEED_LEN, K, st.pos, hps, sets=st.sets, set_of_row=MIXED, image_of_row=IOR)
    finally:
        grp.close(parent=False)
        st.eng.set_image_embeds(st.emb)
    _same(got, want)


def _raw(st, sets, n_sets, set_of_row):
    """the C call itself (the Python wrapper derives n_sets from the table) -> (status, message)"""
    eng = st.eng
    hp = hyper_array([HP() for _ in range(R)])
    ids = np.empty((2, R, st.start.shape[1]), np.int32)
    cos = np.empty((2, R), np.float32)
    so = None if set_of_row is None else np.ascontiguousarray(set_of_row, np.int32)
    rc = eng.lib.czc_generate_rows_vocab(eng.h, R, st.start.shape[1], SEED_LEN, _ptr(st.start), None, _ptr(IOR), None, K, st.pos.shape[0],
                                         _ptr(st.pos), None, L, hp, None, None, 0, None, _ptr(sets), n_sets, _ptr(so), _ptr(ids), _ptr(cos))
    return rc, eng.lib.czc_last_error(eng.h).decode()


def test_refusals(setups):
    st = setups(F32)
    before = st.eng.stats()
    some = np.array([0, -1, 1, -1, 0, 1], np.int32)
    for what, (sets, n_sets, so), names in (
            ("n_sets < 1", (st.sets, 0, some), "n_sets"),
            ("n_sets < 1, all -1", (st.sets, 0, [-1] * R), "n_sets"),
            ("sets NULL", (None, 2, some), "sets"),
            ("index too large", (st.sets, 2, [0, 1, 2, 0, 1, 0]), "set_of_row"),
            ("index below -1", (st.sets, 2, [0, 1, -2, 0, 1, 0]), "set_of_row"),
            ("too many sets", (st.sets, native.MAX_VOCAB_SETS + 1, some), "n_sets")):
        rc, msg = _raw(st, sets, n_sets, so)
        assert rc == native.ERR_ARG, (what, rc, msg)
        assert "generate_rows_vocab" in msg and names in msg, (what, msg)
    assert st.eng.stats() == before   # refused before any GPU work
    # what czc_generate_rows_vs checks is still checked: a rival index outside the resident batch
    with pytest.raises(NativeError) as exc:
        st.vocab([HP() for _ in range(R)], MIXED, rv=np.full((R, 1), N_IMG, np.int32), dl=np.ones(R, np.float32))
    assert exc.value.code == native.ERR_ARG
    # the wrapper refuses a table of the wrong width before the call
    with pytest.raises(ValueError):
        st.vocab([HP() for _ in range(R)], MIXED, sets=st.sets[:, :-1])
    # and the engine is usable: a correct call right after succeeds and returns what it returns
    rc, msg = _raw(st, st.sets, 2, MIXED)
    assert rc == 0, msg
    _same(st.vocab([HP(t) for t in TEMPS], MIXED), st.vocab([HP(t) for t in TEMPS], MIXED))
