"""Options "share_layer0" and "pool_last_qkv": the first and the last CLIP-text layer compute only the rows that differ.

Kernel level, attention_image_kernel's two indirect modes (tests/tower_hooks.py) against the plain per-image kernel on the
same plan (2 images, 8 heads, K = 7: one image whose candidates share one group behind a trunk, one without trunk whose
branches of 1..11 rows make four groups with a partial last one; one candidate without rows):
 * pooled mode: the compact row of every candidate is, bit for bit, what the plain kernel stores at that candidate's last own
   row, a candidate without rows receives its representative's row, nothing else is written; the q columns of the packed
   buffer and the compact q rows of candidates without rows are NaN: the pooled mode reads neither;
 * mapped mode: a q/k/v buffer that holds aliased rows once (identity entries, aliases inside a group, aliases to a row of an
   earlier group) gives the context of the plain kernel on the expanded buffer, bit for bit.
Plan kernels (launch_layer0_count / launch_layer0_map) against a numpy restatement, on ids where two candidates share a token
at one offset and not at the next, candidates of different token counts and a duplicate sentence.

Engine level: the smallest towers on which the folded path and the per-image kernel both run (CLIP-text hidden 512, 8 heads,
2 layers; B = 2, K = 8, per-image kernel forced), under every combination of the two options:
 * hand-made CLIP id tables (mixed token counts, one duplicate sentence, `dedup` on) through the engine's own plan and tower
   (czc_test_text_tower): text features and cosines bitwise equal, and the duplicate is counted;
 * steps and short czc_generate calls on a BERT head that leaves fewer than K live candidates (the rest decode to one
   sentence, so every step carries candidates without rows): bitwise equal, on the bf16 engine and on the screen-then-refine
   engine (whose fp16 screening pass takes the same path).
"""
import numpy as np
import pytest

import kernel_hooks as KH
import tower_hooks as PH
from conzic_amd import harness, native, synth
from conzic_amd.engine import Engine

pytestmark = pytest.mark.gpu

BF16, FP16, REFINE = native.PREC_BF16, native.PREC_FP16, native.PREC_REFINE
SCALE = 0.125
HEADS = 8

# 2 images, K = 7.  Image 0: trunk of 5 rows, longest branch 3 -> G = 10, one group holds all candidates, candidate 3 has no rows
# (a de-duplicated copy of candidate 1).  Image 1: no trunk, branches of 1..11 rows -> G = 2, four groups, the last one partial.
TRUNK = np.array([5, 0], np.int32)
OWN = np.array([[3, 1, 2, 0, 3, 2, 1],
                [1, 11, 4, 7, 2, 9, 5]], np.int32)
REP = {(0, 3): 1}


def _plan_rows():
    """-> (packed row of every candidate's last own row [B, K] with representatives resolved, rows in all)"""
    B, K = OWN.shape
    off = int(TRUNK.sum())
    last = np.zeros((B, K), np.int64)
    for b in range(B):
        for k in range(K):
            off += int(OWN[b, k])
            last[b, k] = off - 1
    for (b, k), r in REP.items():
        assert OWN[b, k] == 0 and OWN[b, r] > 0
        last[b, k] = last[b, r]
    return last, off


@pytest.mark.parametrize("prec", [BF16, FP16], ids=["bf16", "fp16"])
def test_pooled_mode_equals_plain_kernel_rows(prec):
    last, rows = _plan_rows()
    B, K = OWN.shape
    Hd = HEADS * 64
    rng = np.random.default_rng(7)
    qkv = rng.standard_normal((rows, 3 * Hd)).astype(np.float32)
    refused, ref, guard = KH.attention_plan(prec, 2, TRUNK, OWN, HEADS, SCALE, qkv)
    assert not refused
    assert (guard == KH.PLAN_SENTINEL[prec]).all()

    qc = qkv[last.reshape(-1), :Hd].copy()
    for (b, k) in REP:
        qc[b * K + k] = np.nan          # a candidate without rows has no query lane
    poisoned = qkv.copy()
    poisoned[:, :Hd] = np.nan           # the packed q columns are not this mode's to read
    rep = np.tile(np.arange(K), (B, 1))
    for (b, k), r in REP.items():
        rep[b, k] = r
    ctx, cguard = PH.attention_pooled(prec, TRUNK, OWN, rep, HEADS, SCALE, poisoned, qc)
    assert (cguard == KH.PLAN_SENTINEL[prec]).all(), "stray store around the compact context rows"
    assert np.isfinite(ctx).all()
    want = ref[last.reshape(-1)]
    bad = np.nonzero((ctx.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert bad.size == 0, f"compact rows {bad.tolist()} differ from the plain kernel's rows {last.reshape(-1)[bad].tolist()}"


@pytest.mark.parametrize("prec", [BF16, FP16], ids=["bf16", "fp16"])
def test_mapped_mode_equals_plain_kernel_on_expanded_rows(prec):
    _, rows = _plan_rows()
    B, K = OWN.shape
    Hd = HEADS * 64
    ooff = int(TRUNK.sum()) + np.concatenate([[0], np.cumsum(OWN.reshape(-1))])[:-1].reshape(B, K)
    # representative of every packed row: itself unless aliased below (row of candidate k at offset i = ooff[b, k] + i)
    rep = np.arange(rows)
    rep[ooff[0, 2] + 1] = ooff[0, 0] + 1        # image 0 (one group): an alias inside the group
    rep[ooff[0, 4] + 2] = ooff[0, 0] + 2
    rep[ooff[0, 5] + 1] = ooff[0, 0] + 1
    rep[ooff[1, 2] + 0] = ooff[1, 0] + 0        # image 1, group 1 (candidates 2, 3) -> a row of group 0
    rep[ooff[1, 3] + 3] = ooff[1, 1] + 3
    rep[ooff[1, 3] + 1] = ooff[1, 2] + 1        # inside group 1
    rep[ooff[1, 6] + 4] = ooff[1, 1] + 4        # the partial last group -> group 0
    rep[ooff[1, 5] + 8] = ooff[1, 1] + 8        # group 2 -> group 0
    assert (rep[rep] == rep).all() and (rep <= np.arange(rows)).all()
    keep = np.nonzero(rep == np.arange(rows))[0]
    cidx = np.full(rows, -1)
    cidx[keep] = np.arange(keep.size)
    rowmap = cidx[rep]
    assert (rowmap[:int(TRUNK.sum())] == np.arange(int(TRUNK.sum()))).all() and keep.size < rows
    rng = np.random.default_rng(11)
    compact = rng.standard_normal((keep.size, 3 * Hd)).astype(np.float32)
    refused, ref, guard = KH.attention_plan(prec, 2, TRUNK, OWN, HEADS, SCALE, compact[rowmap])
    assert not refused and (guard == KH.PLAN_SENTINEL[prec]).all()
    out, mguard = PH.attention_mapped(prec, TRUNK, OWN, rowmap, HEADS, SCALE, compact)
    assert (mguard == KH.PLAN_SENTINEL[prec]).all(), "stray store around the context rows"
    bad = np.nonzero((out.view(np.uint32) != ref.view(np.uint32)).any(1))[0]
    assert bad.size == 0, f"context rows {bad.tolist()} differ from the plain kernel on the expanded buffer"


def _ids_table():
    """B = 2, K = 7 CLIP id rows [B, K, 77] / lengths: BOS, a two-token common prefix, then per candidate its own tokens and a
    shared suffix, EOS.  Image 0: one-token words except candidates 2 and 5 (two tokens: their suffix shifts and pairs up), 3
    repeats 1 (duplicate sentence), 4 shares its word with 0 but not the token behind it.  Image 1: nothing in common behind BOS."""
    BOS, EOS = 900, 901
    sfx = [50, 51, 52]
    img0 = [[10, 11, 20] + sfx, [10, 11, 21] + sfx, [10, 11, 22, 23] + sfx, [10, 11, 21] + sfx, [10, 11, 20, 60, 51, 52],
            [10, 11, 24, 23] + sfx, [10, 11, 25, 50, 51]]
    img1 = [[30 + k] + [70 + (k % 3)] * (k % 4) + [80, 81][: 1 + k % 2] for k in range(7)]
    ids = np.full((2, 7, 77), EOS, np.int32)
    ln = np.zeros((2, 7), np.int32)
    for b, img in enumerate((img0, img1)):
        for k, body in enumerate(img):
            row = [BOS] + body + [EOS]
            ids[b, k, :len(row)] = row
            ln[b, k] = len(row)
    return ids, ln


def _layer0_ref(ids, own_off, own_len, B, K):
    """numpy restatement: rowmap / dist / per-image distinct counts from the segment table the plan produced"""
    M = int(own_off[-1])
    rep = np.arange(M)
    dcount = np.zeros(B, np.int64)
    for b in range(B):
        pb = int(own_len[b])
        for k in range(K):
            s = B + b * K + k
            for i in range(int(own_len[s])):
                r = int(own_off[s]) + i
                for j in range(k):
                    sj = B + b * K + j
                    if own_len[sj] > i and ids[b, j, pb + i] == ids[b, k, pb + i]:
                        rep[r] = int(own_off[sj]) + i
                        break
                dcount[b] += rep[r] == r
    keep = np.nonzero(rep == np.arange(M))[0]
    cidx = np.full(M, -1)
    cidx[keep] = np.arange(keep.size)
    return cidx[rep], keep, dcount


def test_layer0_plan_matches_numpy():
    ids, ln = _ids_table()
    B, K = ln.shape
    got = PH.layer0_plan(ids, ln, dedup=True)
    own_off, own_len = got["own_off"], got["own_len"]
    assert own_len[B + 3] == 0, "candidate 3 of image 0 repeats candidate 1"
    rowmap, dist, dcount = _layer0_ref(ids, own_off, own_len, B, K)
    assert got["totals"][0] == own_off[-1] and got["totals"][6] == own_off[B]
    np.testing.assert_array_equal(got["dcount"], dcount)
    assert got["totals"][8] == dcount.sum()
    np.testing.assert_array_equal(got["dist"], dist)
    np.testing.assert_array_equal(got["rowmap"], rowmap)
    # the cases the table is there for: shared at one offset and not at the next; two-token words pairing up with one another
    o = own_off[B:B + K]
    assert rowmap[o[4]] == rowmap[o[0]] and rowmap[o[4] + 1] != rowmap[o[0] + 1]
    assert rowmap[o[5] + 1] == rowmap[o[2] + 1] and rowmap[o[5] + 2] == rowmap[o[2] + 2] and rowmap[o[5]] != rowmap[o[2]]
    assert dist.size < own_off[-1]


# ---- engine level ---------------------------------------------------------------------------------------------------------
N_HOT = 5   # live candidates per step of the tiny BERT head below (K = 8: the other three decode to one sentence)


def _peaky_tiny_bert(bcfg, sv):
    """tests/test_step_gpu.py::_peaky_bert_weights on the tiny vocabulary: N_HOT regular tokens far above a bulk that softmax(logits
    / 0.1) sends to exactly zero, so the tail of the top-K is zero-probability fill-ins that all decode to the caption without the word"""
    w = synth.make_bert_weights(bcfg, 11)
    regular = np.nonzero(synth.make_token_mask(sv, regular_only=True)[0] > 0)[0]
    hot = np.random.default_rng(5).choice(regular, size=N_HOT, replace=False)
    bias = w["cls.predictions.bias"].copy()
    bias[hot] += np.linspace(16.0, 5.6, N_HOT).astype(np.float32)
    w["cls.predictions.bias"] = bias
    if "cls.predictions.decoder.bias" in w:
        w["cls.predictions.decoder.bias"] = bias
    return w


@pytest.fixture(scope="module")
def setups():
    made = {}

    def get(prec):
        if prec not in made:
            sv = harness.cached_vocab(True)
            ccfg = synth.clip_tiny(len(sv.clip_vocab))
            ccfg.hidden, ccfg.heads, ccfg.inter, ccfg.layers = 512, 8, 2048, 2
            bcfg = synth.bert_tiny(len(sv.bert_tokens))
            su = harness.build_synthetic(True, prec, clip_cfg=ccfg, bert_cfg=bcfg, bert_w=_peaky_tiny_bert(bcfg, sv))
            su.emb = np.random.default_rng(3).standard_normal((2, ccfg.proj)).astype(np.float32)
            su.engine.set_image_embeds(su.emb)
            made[prec] = su
        return made[prec]

    yield get
    for su in made.values():
        su.engine.close()


@pytest.fixture
def per_image_kernel():
    lib = native.load_test()
    assert lib.czc_test_set_option(b"attention_image", 2) == 0
    yield
    lib.czc_test_set_option(b"attention_image", 1)


def _init(su, L):
    prompt = "Image of a"
    return np.array(su.bert_tok.encode(prompt + su.bert_tok.mask_token * L), dtype=np.int32), len(prompt.split()) + 1


OPTS = [(0, 0), (1, 0), (0, 1), (1, 1)]   # (share_layer0, pool_last_qkv)


def _set(eng, share, pool):
    eng.set_option("share_layer0", share)
    eng.set_option("pool_last_qkv", pool)


def _tower_ids(ccfg):
    """_ids_table with the tower's own BOS / EOS, ids inside its vocabulary and an eighth candidate per image (K = 8)"""
    ids, ln = _ids_table()
    B, K0 = ln.shape
    K = K0 + 1
    out = np.full((B, K, 77), ccfg.eos_id, np.int32)
    oln = np.zeros((B, K), np.int32)
    for b in range(B):
        for k in range(K):
            src = ids[b, min(k, K0 - 1)].copy()
            n = int(ln[b, min(k, K0 - 1)])
            if k == K0:                       # a candidate of its own: another word in front of candidate 6's suffix
                src[1 if b else 3] = 40 + b
            body = src[1:n - 1] % (ccfg.vocab - 2)
            out[b, k, 0] = ccfg.bos_id
            out[b, k, 1:n - 1] = body
            oln[b, k] = n
    return out, oln


def test_hand_made_ids_through_the_tower_under_every_option_pair(setups, per_image_kernel):
    su = setups(BF16)
    eng = su.engine
    ids, ln = _tower_ids(su.clip_cfg)
    B, K = ln.shape
    assert K == 8 and len(set(ln[0].tolist())) > 1 and (ids[0, 3] == ids[0, 1]).all() and eng.get_option("dedup") == 1
    outs = []
    try:
        for share, pool in OPTS:
            _set(eng, share, pool)
            eng.profile(1)
            eng.profile_reset()
            feat, n_dup = PH.text_tower(eng, ids, ln)
            flops = eng.profile_get("gemm_clip_text")
            eng.profile(0)
            assert n_dup == 1, "candidate 3 of image 0 repeats candidate 1"
            outs.append((feat, eng.similarity(su.emb, feat, K), flops))
    finally:
        _set(eng, 1, 1)
        eng.profile(0)
    # the paths under test ran: one more GEMM launch with the pooled last layer, fewer rows multiplied with layer 0 on distinct rows
    assert outs[2][2]["launches"] == outs[0][2]["launches"] + 1 and outs[3][2]["launches"] == outs[1][2]["launches"] + 1
    assert outs[1][2]["flops"] < outs[0][2]["flops"] and outs[3][2]["flops"] < outs[2][2]["flops"]
    f0, (s0, c0), _ = outs[0]
    assert np.isfinite(f0).all()
    assert f0[3].tobytes() == f0[1].tobytes(), "the duplicate carries its representative's feature"
    for feat, (cs, cr), _ in outs[1:]:
        assert feat.tobytes() == f0.tobytes()
        assert cs.tobytes() == s0.tobytes() and cr.tobytes() == c0.tobytes()


def test_step_is_bitwise_equal_under_every_option_pair(setups, per_image_kernel):
    su = setups(BF16)
    eng = su.engine
    assert eng.get_option("pool_last_qkv") == 1 and eng.get_option("share_layer0") == 1 and eng.get_option("has_folded_ln_weights") == 1
    init, seed_len = _init(su, 4)
    hp = Engine.hyper(0.02, 2.0, 0.1)
    B, K = 2, 8
    outs, launches, dups = [], [], []
    try:
        for share, pool in OPTS:
            _set(eng, share, pool)
            eng.profile(1)
            eng.profile_reset()
            d0 = eng.stats()["dedup_seqs"]
            inp = np.ascontiguousarray(np.tile(init, (B, 1)))
            res = []
            for gi in (seed_len, seed_len + 2, seed_len + 3, seed_len + 1):   # later steps: filled captions, mixed token counts
                res.append(eng.step(inp, gi, K, hp, dot_allowed=(gi == seed_len + 3)))
            outs.append(res)
            launches.append((eng.profile_get("gemm_clip_text")["launches"], eng.profile_get("attention_clip_text")["launches"],
                             eng.profile_get("gemm_clip_text")["flops"]))
            dups.append(eng.stats()["dedup_seqs"] - d0)
            eng.profile(0)
    finally:
        _set(eng, 1, 1)
        eng.profile(0)
    # the paths under test ran: the pooled last layer splits its q/k/v GEMM in two launches per step (4 steps), layer 0 on
    # distinct rows multiplies fewer rows
    assert launches[2][0] == launches[0][0] + 4 and launches[3][0] == launches[1][0] + 4, launches
    assert launches[1][2] < launches[0][2] and launches[3][2] < launches[2][2], launches
    assert all(l[1] == launches[0][1] for l in launches), launches
    # every step carries K - N_HOT candidates of one sentence per image: all but the first of them have no rows of their own
    assert dups[0] >= 4 * B * (K - N_HOT - 1) and all(d == dups[0] for d in dups), dups
    lens = np.concatenate([r["clip_len"] for r in outs[0]])
    assert len(set(lens.tolist())) > 1, "the candidates of the steps should differ in their CLIP token counts"
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            for name in ("clip_ids", "clip_len", "clip_ref", "clip_score", "final_score", "best", "best_cos"):
                assert a[name].tobytes() == b[name].tobytes(), name


@pytest.mark.parametrize("prec", [BF16, REFINE], ids=["bf16", "refine"])
def test_generate_is_bitwise_equal_under_every_option_pair(prec, setups, per_image_kernel):
    su = setups(prec)
    eng = su.engine
    L, B, K = 3, 2, 8
    init, seed_len = _init(su, L)
    hp = Engine.hyper(0.02, 2.0, 0.1)
    positions = list(range(L)) * 2
    outs, dups = [], []
    try:
        for share, pool in OPTS:
            _set(eng, share, pool)
            d0 = eng.stats()["dedup_seqs"]
            outs.append(eng.generate(B, init, L, seed_len, K, positions, hp))
            dups.append(eng.stats()["dedup_seqs"] - d0)
    finally:
        _set(eng, 1, 1)
    assert dups[0] >= len(positions) * B * (K - N_HOT - 1) and all(d == dups[0] for d in dups), dups
    for ids, cos in outs[1:]:
        assert ids.tobytes() == outs[0][0].tobytes()
        assert cos.tobytes() == outs[0][1].tobytes()
    assert np.isfinite(outs[0][1]).all()
