"""-m gpu: the per-row forms of the top-K selection (conzic_amd/csrc/topk.hip) -- launch_softmax_mask_topk_rows (the '.' rule per
row) and launch_softmax_mask_topk_rows_hp (the temperature per row as well) -- launched alone through czc_test_topk_rows.

Reference: softmax(logits / temperature_row) in fp64, times the mask with '.' by dot_rows[b], ordered by (probability descending, id
ascending).  The logits are built so that the order is certain -- a hot set of K + 20 ids above a random bulk, neighbouring fp64
probabilities more than 1e-4 apart relatively (asserted from the reference; the kernel's fp32 error is below 2e-5, see below) --
so the ids are compared exactly at every place; planted exact ties (equal logits) must come out in ascending id, one of them
across the K-th place, where only the lower id is taken.

Magnitudes: |logit| <= 1.05 and temperature >= 0.05 keep |logit / T| <= 21, so that the fp32 quotient and the subtraction of the
row maximum are off by at most 2 * 21 * 2^-24 = 2.5e-6 in the exponent, i.e. relatively in the probability; expf, the sum and
the division add a few 2^-24.  The probabilities are held to rtol 2e-5, the bound of test_softmax_mask_topk.
"""
import numpy as np
import pytest

import kernel_hooks as KH
from conzic_amd import native

pytestmark = pytest.mark.gpu

B = 6
DOT_ROWS = np.array([1, 0, 1, 0, 1, 0], np.int32)
TEMPS = [0.05, 0.1, 1.0, 3.0, 0.05, 1.0]
SHAPES = [(640, 12), (30522, 200)]


def build(V, K):
    """-> logits [B, V], mask [V], dot_id, ties: {row: [(lower id, higher id)]}"""
    rng = np.random.default_rng(V * 31 + K)
    logits = np.clip(rng.standard_normal((B, V)) * 0.02, -0.1, 0.1).astype(np.float32)
    mask = np.ones(V, np.float32)
    mask[rng.choice(V, size=V // 10, replace=False)] = 0.0
    dot_id = 17
    mask[dot_id] = 0.0           # the row's rule replaces the mask's entry, either way
    n_hot = K + 20
    hots = [rng.choice(np.setdiff1d(np.arange(V), [0, dot_id]), size=n_hot, replace=False) for _ in range(B)]
    for hot in hots:
        mask[hot] = 1.0
    for hot in hots:             # five masked ids inside every hot set, two of them near the K-th place: they must drop out
        mask[hot[[3, 9, K // 2 + 4, K - 2, K + 5]]] = 0.0
    ties = {}
    for b, hot in enumerate(hots):
        logits[b, hot] = np.linspace(1.0, 0.2, n_hot).astype(np.float32)
        logits[b, dot_id] = 1.05  # the row maximum
        live = hot[mask[hot] > 0]   # in descending order of their logits
        assert live.size >= K + 2 and live.size < n_hot
        # an exact tie in the middle of the selection, and (odd rows) one across the K-th place ('.' takes a place where allowed)
        pairs = [(K // 2, K // 2 + 1)] + ([(K - 1 - DOT_ROWS[b], K - DOT_ROWS[b])] if b % 2 else [])
        ties[b] = []
        for i, j in pairs:
            logits[b, live[j]] = logits[b, live[i]]
            ties[b].append(tuple(sorted((int(live[i]), int(live[j])))))
    return logits, mask, dot_id, ties


def reference(logits, mask, dot_id, dot_rows, temps, K):
    """fp64 -> (probs [B, K], ids [B, K], full probability rows [B, V], mask rows [B, V])"""
    x = logits.astype(np.float64) / np.array(temps, np.float32).astype(np.float64)[:, None]
    p = np.exp(x - x.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    mk = np.tile(mask.astype(np.float64), (logits.shape[0], 1))
    mk[:, dot_id] = dot_rows
    p *= mk
    order = np.lexsort((np.arange(p.shape[1])[None, :].repeat(p.shape[0], 0), -p), axis=1)[:, :K]
    return np.take_along_axis(p, order, 1), order, p, mk


def hyper_rows(temps):
    return [native.Hyper(0.02, 2.0, 0.0, float(t), 0, 0) for t in temps]


def launch(form, logits, mask, K, dot_id, temps):
    if form == 1:
        return KH.topk_rows(1, logits, mask, K, dot_id, DOT_ROWS, temperature=temps[0])
    return KH.topk_rows(2, logits, mask, K, dot_id, DOT_ROWS, hyper=hyper_rows(temps))


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("V,K", SHAPES)
def test_rows_forms_against_fp64(V, K, form):
    logits, mask, dot_id, ties = build(V, K)
    temps = [0.1] * B if form == 1 else TEMPS
    rp, ri, p, mk = reference(logits, mask, dot_id, DOT_ROWS, temps, K)
    # the order is certain: neighbours among the first K + 1 are more than 1e-4 apart, the planted ties aside (and those are exact)
    for b in range(B):
        top = np.lexsort((np.arange(V), -p[b]))[:K + 1]
        tied = {frozenset(t) for t in ties[b]}
        for a, c in zip(top[:-1], top[1:]):
            if frozenset((int(a), int(c))) in tied:
                assert p[b, a] == p[b, c] and a < c
            else:
                assert p[b, a] - p[b, c] > 1e-4 * p[b, a], (b, a, c)
        assert all(lo in ri[b] for lo, _ in ties[b]) and (b % 2 == 0 or ties[b][1][1] not in ri[b])   # the tie across the K-th place
        assert (ri[b, 0] == dot_id) == bool(DOT_ROWS[b]) and (dot_id in ri[b]) == bool(DOT_ROWS[b])     # '.' leads where allowed
    refused, g = launch(form, logits, mask, K, dot_id, temps)
    assert not refused
    g.assert_guards()
    np.testing.assert_array_equal(g["idxs"], ri)
    np.testing.assert_allclose(g["probs"], rp, rtol=2e-5, atol=0)
    np.testing.assert_array_equal(g["cand"], (g["idxs"] * np.take_along_axis(mk, g["idxs"].astype(np.int64), 1)).astype(np.int32))
    assert (g["cand"] > 0).all()   # nothing masked was selected ('.' would be 0 = [PAD] in a row that does not allow it)
    # on top of the reference: a row's outputs are those of the scalar-form launch with the row's own parameters, bit for bit
    for b in range(B):
        sp, si, sc = KH.topk(logits[b:b + 1], mask, K, temps[b], dot_id, bool(DOT_ROWS[b]))
        assert np.array_equal(sp.view(np.uint32)[0], g["probs"].view(np.uint32)[b]) and np.array_equal(si[0], g["idxs"][b])
        assert np.array_equal(sc[0], g["cand"][b])


@pytest.mark.parametrize("missing", ["hp_rows", "dot_rows"])
def test_hp_form_refuses_missing_arguments(missing):
    V, K = SHAPES[0]
    logits, mask, dot_id, _ = build(V, K)
    refused, g = KH.topk_rows(2, logits, mask, K, dot_id, None if missing == "dot_rows" else DOT_ROWS,
                              hyper=None if missing == "hp_rows" else hyper_rows(TEMPS))
    assert refused
    g.assert_guards()
    for name in ("probs", "idxs", "cand"):
        assert KH.untouched(g[name]).all(), name
