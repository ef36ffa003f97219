"""-m gpu: the top-K selection with a vocabulary set per row (conzic_amd/csrc/topk.hip, the VOCAB instantiation of
softmax_mask_topk_kernel behind launch_softmax_mask_topk_rows_vocab), launched alone through czc_test_topk_rows_vocab.

B = 6 rows with set indices [-1, 0, 1, 2, 1, -1], a '.' rule and a temperature per row.  The sets:
  set 0  bans a tenth of the ids (at least five): five of them inside the hot set of the row that carries it, two of those next to
         the K-th place;
  set 1  an allow-list of K + 10 ids;
  set 2  an allow-list of K - 2 ids, so that [PAD] candidates must appear, at probability 0 and in ascending id.

(a) the outputs are, row by row and bit for bit, those of czc_test_topk_rows form 2 (launch_softmax_mask_topk_rows_hp) run once per
    distinct set with mask * bits multiplied on the host: the defining property of czc_generate_rows_vocab at the kernel.
(b) against fp64, the construction and the bars of tests/test_topk_rows_gpu.py: softmax(logits / temperature_row) times the row's
    mask factors, ordered by (probability descending, id ascending).  A hot set of K + 20 ids -- one set of ids for all rows, so
    that the construction fits V = 33, in a row's own order -- sits above a random bulk; neighbouring fp64 probabilities among a
    row's first K + 1 are either exactly equal (the planted ties, and the zeros of set 2) or more than 1e-4 apart relatively
    (asserted), so the ids are compared exactly.  |logit| <= 1.05 and temperature >= 0.05 keep |logit / T| <= 21: the fp32 quotient
    and the subtraction of the row maximum are off by at most 2 * 21 * 2^-24 = 2.5e-6 in the exponent, expf, the sum and the
    division add a few 2^-24, and the probabilities are held to rtol 2e-5.

V covers the edges of the 32-bit words of a set (33, 64, 65), a size with several elements per thread (1025) and the product's
30 522; K in {1, 5, 200} wherever the hot set fits.
"""
import numpy as np
import pytest

import kernel_hooks as KH
import vocab_hooks as VH
from conzic_amd import native, vocab

pytestmark = pytest.mark.gpu

B = 6
DOT_ROWS = np.array([1, 0, 1, 0, 1, 0], np.int32)
TEMPS = [0.05, 0.1, 1.0, 3.0, 0.05, 1.0]
SET_ROWS = np.array([-1, 0, 1, 2, 1, -1], np.int32)
SHAPES = [(V, K) for V in (33, 64, 65, 1025, 30522) for K in (1, 5, 200) if K + 20 <= V - 2]


def hyper_rows(temps):
    return [native.Hyper(0.02, 2.0, 0.0, float(t), 0, 0) for t in temps]


def five_of(places, n):
    """the first five distinct values of `places`, clipped to [0, n)"""
    out = []
    for i in np.clip(places, 0, n - 1):
        if int(i) not in out and len(out) < 5:
            out.append(int(i))
    assert len(out) == 5
    return out


def build(V, K):
    """-> logits [B, V], mask [V], dot_id, ties {row: [(lower id, higher id)]}, lives [B][..] (a row's unmasked hot ids in
    descending order of their logits), bits uint32 [3, W]"""
    rng = np.random.default_rng(V * 31 + K)
    logits = np.clip(rng.standard_normal((B, V)) * 0.02, -0.1, 0.1).astype(np.float32)
    mask = np.ones(V, np.float32)
    dot_id = 17
    mask[dot_id] = 0.0           # the row's rule replaces the mask's entry, either way
    n_hot = K + 20
    pool = np.setdiff1d(np.arange(V), [0, dot_id])
    hot_ids = rng.choice(pool, size=n_hot, replace=False)
    rest = np.setdiff1d(pool, hot_ids)
    mask[rng.choice(rest, size=min(rest.size, V // 10), replace=False)] = 0.0
    mask[hot_ids[five_of([3, 9, K // 2 + 4, K - 2, K + 5, 12, 14, 16], n_hot)]] = 0.0   # five stop words inside the hot set
    ties, lives = {}, []
    for b in range(B):
        hot = hot_ids[rng.permutation(n_hot)]
        logits[b, hot] = np.linspace(1.0, 0.2, n_hot).astype(np.float32)
        logits[b, dot_id] = 1.05  # the row maximum
        live = hot[mask[hot] > 0]
        assert live.size == K + 15
        # an exact tie in the middle of the selection, and (odd rows) one across the K-th place ('.' takes a place where allowed)
        pairs = [(K // 2, K // 2 + 1)] + ([(K - 1 - DOT_ROWS[b], K - DOT_ROWS[b])] if b % 2 else [])
        ties[b] = []
        for i, j in pairs:
            logits[b, live[j]] = logits[b, live[i]]
            ties[b].append(tuple(sorted((int(live[i]), int(live[j])))))
        lives.append(live)
    # set 0, carried by row 1: five bans inside its live hot ids, two of them next to its K-th place; then up to a tenth of the ids
    ban = set(int(i) for i in lives[1][five_of([K - 2, K, 2, 6, K // 2 + 2, 8, 10, 11], K + 15)])
    for i in rng.permutation(rest):
        if len(ban) >= max(V // 10, 5):
            break
        ban.add(int(i))
    allowed0 = np.ones(V, bool)
    allowed0[sorted(ban)] = False
    assert allowed0[dot_id]      # '.' is inside set 0: row 1's rule must still keep it out
    set1 = lives[2][:K + 10]     # '.' is outside sets 1 and 2: the rule of rows 2 and 4 must still bring it in
    set2 = lives[3][:max(K - 2, 0)]
    bits = vocab.pack([allowed0, set1, set2], V)
    return logits, mask, dot_id, ties, lives, bits


def mask_rows(mask, bits, set_rows, V):
    """[B, V]: mask * bit of the row's set (the '.' entry is overridden by the caller's rule)"""
    allowed = vocab.unpack(bits, V)
    return np.stack([mask * (allowed[s] if s >= 0 else 1.0) for s in set_rows]).astype(np.float32)


def reference(logits, mk_rows, dot_id, dot_rows, temps, K):
    """fp64 -> (probs [B, K], ids [B, K], full probability rows [B, V], mask rows [B, V])"""
    x = logits.astype(np.float64) / np.array(temps, np.float32).astype(np.float64)[:, None]
    p = np.exp(x - x.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    mk = mk_rows.astype(np.float64)
    mk[:, dot_id] = dot_rows
    p *= mk
    order = np.lexsort((np.arange(p.shape[1])[None, :].repeat(p.shape[0], 0), -p), axis=1)[:, :K]
    return np.take_along_axis(p, order, 1), order, p, mk


_cases = {}


def case(V, K):
    """the inputs of a shape and its one launch of the kernel under test, shared by the tests (read only)"""
    if (V, K) not in _cases:
        logits, mask, dot_id, ties, lives, bits = build(V, K)
        refused, g = VH.topk_rows_vocab(logits, mask, K, dot_id, DOT_ROWS, hyper_rows(TEMPS), SET_ROWS, bits)
        assert not refused
        g.assert_guards()
        _cases[(V, K)] = (logits, mask, dot_id, ties, lives, bits, g)
    return _cases[(V, K)]


@pytest.mark.parametrize("V,K", SHAPES)
def test_rows_equal_the_hp_form_under_the_premultiplied_mask(V, K):
    logits, mask, dot_id, _, _, bits, g = case(V, K)
    allowed = vocab.unpack(bits, V)
    for s in (-1, 0, 1, 2):
        m = mask if s < 0 else (mask * allowed[s]).astype(np.float32)
        refused, h = KH.topk_rows(2, logits, m, K, dot_id, DOT_ROWS, hyper=hyper_rows(TEMPS))
        assert not refused
        rows = np.nonzero(SET_ROWS == s)[0]
        assert rows.size
        for name in ("probs", "idxs", "cand"):
            assert np.array_equal(g[name][rows].view(np.uint32), h[name][rows].view(np.uint32)), (s, name)


@pytest.mark.parametrize("V,K", SHAPES)
def test_rows_against_fp64(V, K):
    logits, mask, dot_id, ties, lives, bits, g = case(V, K)
    rp, ri, p, mk = reference(logits, mask_rows(mask, bits, SET_ROWS, V), dot_id, DOT_ROWS, TEMPS, K)
    for b in range(B):   # the order is certain: neighbours among the first K + 1 are exactly equal or more than 1e-4 apart
        top = np.lexsort((np.arange(V), -p[b]))[:K + 1]
        for a, c in zip(top[:-1], top[1:]):
            assert (p[b, a] == p[b, c] and a < c) or p[b, a] - p[b, c] > 1e-4 * p[b, a], (b, a, c)
    for b in (0, 5):     # rows without a set: the planted ties, one of them (odd rows) across the K-th place
        assert K < 5 or (ties[b][0][0] in ri[b] and ties[b][0][1] in ri[b])   # (K = 1 has no room for a tie inside the selection)
        assert b % 2 == 0 or (ties[b][1][0] in ri[b] and ties[b][1][1] not in ri[b])
    np.testing.assert_array_equal(g["idxs"], ri)
    np.testing.assert_allclose(g["probs"], rp, rtol=2e-5, atol=0)
    np.testing.assert_array_equal(g["cand"], (g["idxs"] * np.take_along_axis(mk, g["idxs"].astype(np.int64), 1)).astype(np.int32))
    allowed = vocab.unpack(bits, V)
    # '.' and the sets: the rule decides, whatever the set says
    assert allowed[0][dot_id] and not DOT_ROWS[1] and dot_id not in g["idxs"][1]
    for b in (2, 4):
        assert not allowed[1][dot_id] and DOT_ROWS[b] and g["idxs"][b, 0] == dot_id and g["cand"][b, 0] == dot_id
    # set 0: none of its bans was proposed, and the bans next to the K-th place made room for the ids behind them
    assert allowed[0][g["idxs"][1]].all() and (g["cand"][1] > 0).all()
    assert not allowed[0][lives[1][:K + 1]].all()
    # set 1: K + 10 ids for K places ('.' takes one in rows 2 and 4): every other candidate is of the list
    for b in (2, 4):
        assert allowed[1][g["idxs"][b, 1:]].all() and (g["cand"][b] > 0).all()
    # set 2: K - 2 ids, then [PAD] candidates at probability 0 in ascending id
    n2 = max(K - 2, 0)
    assert allowed[2][g["idxs"][3, :n2]].all() and (g["probs"][3, :n2] > 0).all() and (g["cand"][3, :n2] > 0).all()
    assert (g["probs"][3, n2:] == 0).all() and (g["cand"][3, n2:] == 0).all() and (np.diff(g["idxs"][3, n2:]) > 0).all()
    assert np.array_equal(g["idxs"][3, n2:], np.setdiff1d(np.arange(V), lives[3][:n2])[:K - n2])


@pytest.mark.parametrize("V,K", [s for s in SHAPES if s[0] % 32])
def test_bits_above_the_vocabulary_are_ignored(V, K):
    logits, mask, dot_id, _, _, bits, g = case(V, K)
    dirty = bits.copy()
    dirty[:, -1] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)
    assert (dirty != bits).any() and np.array_equal(vocab.unpack(dirty, V), vocab.unpack(bits, V))
    refused, h = VH.topk_rows_vocab(logits, mask, K, dot_id, DOT_ROWS, hyper_rows(TEMPS), SET_ROWS, dirty)
    assert not refused
    h.assert_guards()
    for name in ("probs", "idxs", "cand"):
        assert np.array_equal(g[name].view(np.uint32), h[name].view(np.uint32)), name


@pytest.mark.parametrize("missing", ["hp_rows", "dot_rows", "set_rows", "bits"])
def test_vocab_form_refuses_missing_arguments(missing):
    V, K = SHAPES[1]
    logits, mask, dot_id, _, _, bits = build(V, K)
    refused, g = VH.topk_rows_vocab(logits, mask, K, dot_id, None if missing == "dot_rows" else DOT_ROWS,
                                    None if missing == "hp_rows" else hyper_rows(TEMPS),
                                    None if missing == "set_rows" else SET_ROWS, None if missing == "bits" else bits)
    assert refused
    g.assert_guards()
    for name in ("probs", "idxs", "cand"):
        assert KH.untouched(g[name]).all(), name
