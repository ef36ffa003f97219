"""fp64 references of the attention kernels (csrc/attention.hip) for tests/: the per-sequence formula, and the
shared-prefix plan the CLIP-text tower runs (B trunk segments, then B*K branch segments back to back).

TEST INFRASTRUCTURE, numpy / torch on the CPU only.  A plan is (trunk_len [B], own_len [B, K]): query i of branch (b, k) sees
trunk keys 0..p_b-1 of image b and own keys 0..i of candidate (b, k); trunk query i sees trunk keys 0..i.  plan_ref() states
that directly (one masked einsum per image over candidates padded to the image's longest branch); test_attn_ref_cpu.py holds
it to seq_ref() on the materialised sequences.  It also carries what the plan tests need around the reference: the three
mask-widening mutants (a reference that is wrong by exactly one key), the rounding model that sets the tolerance where the
inputs are not standard normal, and the constructions of those inputs (bait keys, spotlight queries).

The same for plain segments in both mask modes (seg_ref and the seg_* constructions at the end: what launch_attention serves
for the BERT and vision towers, tests/test_attention_seq_gpu.py): mutants "next" / "prev" / "dup_last", bait by segment parity,
spotlights on either side of the 32-key tile edges, and the twin input on which a last key counted twice shows.
"""
import numpy as np
import torch

F32, BF16, SPLIT, FP16 = 1, 0, 3, 4   # internal precision codes (csrc/common.h PREC_*)
PREC_NAME = {F32: "f32", BF16: "bf16", SPLIT: "split-fp16", FP16: "fp16"}
# the bounds of test_attention_packed_sequences / test_fp16_attention / test_split_fp16_mfma_attention: same arithmetic,
# same input distribution (standard normal q, k, v; scale 0.125)
NORMAL_TOL = {F32: 2e-5, BF16: 1.5e-2, FP16: 2e-3, SPLIT: 3e-5}
# spacing of the output type at the bottom of a binade, relative to the value: bf16 keeps 8 significant bits, fp16 11,
# fp32 (and the hi + lo fp16 planes of the split type, ~22 bits) 24 / 22
ULP = {BF16: 2.0 ** -8, FP16: 2.0 ** -11, F32: 2.0 ** -24, SPLIT: 2.0 ** -22}


def bf16_round(a):
    """round-to-nearest-even to bf16, returned in the input's float width"""
    a32 = np.ascontiguousarray(a, np.float32)
    u = a32.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32).reshape(a32.shape)


def round_operand(prec, a):
    """what the kernel of `prec` reads of fp32 host data: bf16 / fp16 rounding; fp32 and split-fp16 keep the fp32 value
    (the split type holds ~22 bits of it; test_split_fp16_mfma_attention compares against the unrounded operands too)"""
    a = np.ascontiguousarray(a, np.float32)
    if prec == BF16:
        return bf16_round(a)
    if prec == FP16:
        return a.astype(np.float16).astype(np.float32)
    return a


def _round64(prec, a):
    """fp64 array rounded to the storage type of `prec` (the rounding model's P and output)"""
    if prec == BF16:
        return bf16_round(a.astype(np.float32)).astype(np.float64)
    if prec == FP16:
        return a.astype(np.float16).astype(np.float64)
    return a.astype(np.float32).astype(np.float64)


def seq_ref(qkv, lens, heads, causal, scale, dtype=np.float32):
    """softmax(q k^T * scale [+ causal mask]) v per packed sequence; qkv [sum(lens), 3*heads*64], computed in `dtype`"""
    Hd = heads * 64
    qkv = np.ascontiguousarray(qkv, dtype)
    out = np.zeros((qkv.shape[0], Hd), dtype)
    o = 0
    for L in lens:
        blk = torch.from_numpy(qkv[o:o + L])
        q, k, v = blk[:, :Hd], blk[:, Hd:2 * Hd], blk[:, 2 * Hd:]
        q = q.view(L, heads, 64).transpose(0, 1)
        k = k.view(L, heads, 64).transpose(0, 1)
        v = v.view(L, heads, 64).transpose(0, 1)
        s = q @ k.transpose(-1, -2) * scale
        if causal:
            s = s + torch.full((L, L), float("-inf"), dtype=s.dtype).triu(1)
        out[o:o + L] = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(L, Hd).numpy()
        o += L
    return out


def plan_layout(trunk_len, own_len):
    """row offsets of the engine's layout: trunks first, then the branches back to back.  -> trunk_off [B], own_off [B, K], rows"""
    trunk_len = np.asarray(trunk_len, np.int64)
    own_len = np.asarray(own_len, np.int64)
    lens = np.concatenate([trunk_len, own_len.reshape(-1)])
    off = np.concatenate([[0], np.cumsum(lens)])
    B = trunk_len.size
    return off[:B].copy(), off[B:-1].reshape(own_len.shape).copy(), int(off[-1])


def plan_rows(trunk_len, own_len):
    """per plan row: image, candidate (-1 for a trunk row), position inside its segment"""
    trunk_len = np.asarray(trunk_len, np.int64)
    own_len = np.asarray(own_len, np.int64)
    B, K = own_len.shape
    img = np.concatenate([np.repeat(np.arange(B), trunk_len), np.repeat(np.repeat(np.arange(B), K), own_len.reshape(-1))])
    cand = np.concatenate([np.full(int(trunk_len.sum()), -1), np.repeat(np.tile(np.arange(K), B), own_len.reshape(-1))])
    lens = np.concatenate([trunk_len, own_len.reshape(-1)])
    start = np.repeat(np.cumsum(lens) - lens, lens)
    pos = np.arange(int(lens.sum())) - start
    return img, cand, pos


def plan_ref(qkv, trunk_len, own_len, heads, scale, mutant=None, model=None, want_weight=None):
    """fp64 context rows [rows, heads*64] of a shared-prefix plan from operands already rounded to the operand type.

    mutant: None, or a mask that is wrong by ONE key (the proof that a test can fail): "next" -- a query of candidate (b, k)
    also sees own key 0 of candidate (b, k+1); "future" -- query i also sees own key i+1; "other" -- every query of image b
    also sees trunk key 0 of image (b+1) % B.
    model: None, or a precision code: the rounding model -- exp(s - max) rounded to that storage type before the P V product
    (the sum taken from the unrounded values, as the kernels do) and the result rounded to it.
    want_weight: None, or a [rows] array of key indices (position in the query's own key list: trunk keys first, then own
    keys): also returns the softmax weight [rows, heads] each query puts on that key."""
    trunk_len = np.asarray(trunk_len, np.int64)
    own_len = np.asarray(own_len, np.int64)
    B, K = own_len.shape
    Hd = heads * 64
    toff, ooff, rows = plan_layout(trunk_len, own_len)
    x = np.ascontiguousarray(qkv, np.float64).reshape(rows, 3, heads, 64)
    out = np.zeros((rows, heads, 64), np.float64)
    wout = np.zeros((rows, heads), np.float64) if want_weight is not None else None

    def attend(q, keys, vals, mask, tgt):
        # q [S, n, h, d]; keys / vals [S, m, h, d]; mask [S, n, m]; -> [S, n, h, d] (rows without a visible key are padding: 0)
        s = np.einsum("snhd,smhd->shnm", q, keys) * scale
        s = np.where(mask[:, None], s, -np.inf)
        mx = s.max(-1, keepdims=True)
        mx = np.where(np.isfinite(mx), mx, 0.0)
        e = np.exp(s - mx)
        den = e.sum(-1, keepdims=True)
        den = np.where(den > 0, den, 1.0)
        w = None
        if tgt is not None:
            w = np.take_along_axis(e / den, tgt[:, None, :, None].repeat(heads, 1), -1)[..., 0].transpose(0, 2, 1)
        if model is not None:
            e = _round64(model, e)
        o = np.einsum("shnm,smhd->snhd", e, vals) / den.transpose(0, 2, 1, 3)
        if model is not None:
            o = _round64(model, o)
        return o, w

    for b in range(B):
        p = int(trunk_len[b])
        tk = x[toff[b]:toff[b] + p, 1]
        tv = x[toff[b]:toff[b] + p, 2]
        if p:  # the trunk: one causal sequence
            m = np.tril(np.ones((p, p), bool))
            tgt = None if want_weight is None else want_weight[toff[b]:toff[b] + p][None]
            if mutant == "future":
                m = np.tril(np.ones((p, p), bool), 1)
            if mutant == "other" and trunk_len[(b + 1) % B] > 0:
                r = toff[(b + 1) % B]
                tk_m, tv_m = np.concatenate([tk, x[r:r + 1, 1]]), np.concatenate([tv, x[r:r + 1, 2]])
                m = np.concatenate([m, np.ones((p, 1), bool)], 1)
                o, w = attend(x[None, toff[b]:toff[b] + p, 0], tk_m[None], tv_m[None], m[None], tgt)
            else:
                o, w = attend(x[None, toff[b]:toff[b] + p, 0], tk[None], tv[None], m[None], tgt)
            out[toff[b]:toff[b] + p] = o[0]
            if w is not None:
                wout[toff[b]:toff[b] + p] = w[0]
        n = int(own_len[b].max())
        if n == 0:
            continue
        ln = own_len[b]
        idx = ooff[b][:, None] + np.arange(n)[None]               # [K, n] plan rows, padded
        valid = np.arange(n)[None] < ln[:, None]                  # [K, n]
        idx = np.where(valid, idx, 0)
        own = x[idx]                                              # [K, n, 3, h, d]
        keys = [np.broadcast_to(tk[None], (K,) + tk.shape), own[:, :, 1]]
        vals = [np.broadcast_to(tv[None], (K,) + tv.shape), own[:, :, 2]]
        reach = 1 if mutant == "future" else 0
        causal = np.arange(n)[None, :] <= np.arange(n)[:, None] + reach   # [query i, key m]
        mask = [np.ones((K, n, p), bool), causal[None] & valid[:, None, :]]
        if mutant == "next":   # own key 0 of the next candidate of the image, where there is one
            nk = np.roll(own[:, :1], -1, axis=0)
            has = np.roll(ln > 0, -1)
            has[-1] = False
            keys.append(nk[:, :, 1]); vals.append(nk[:, :, 2])
            mask.append(np.broadcast_to(has[:, None, None], (K, n, 1)))
        if mutant == "other" and trunk_len[(b + 1) % B] > 0:
            r = toff[(b + 1) % B]
            keys.append(np.broadcast_to(x[None, r:r + 1, 1], (K, 1, heads, 64)))
            vals.append(np.broadcast_to(x[None, r:r + 1, 2], (K, 1, heads, 64)))
            mask.append(np.ones((K, n, 1), bool))
        mask = np.concatenate(mask, -1) & valid[:, :, None]
        tgt = None
        if want_weight is not None:
            tgt = np.where(valid, want_weight[idx], 0)
        o, w = attend(own[:, :, 0], np.concatenate(keys, 1), np.concatenate(vals, 1), mask, tgt)
        out[idx[valid]] = o[valid]
        if w is not None:
            wout[idx[valid]] = w[valid]
    out = out.reshape(rows, Hd)
    return (out, wout) if want_weight is not None else out


def materialise(qkv, trunk_len, own_len):
    """every trunk and every candidate as a full sequence (trunk rows + own rows): packed rows, lengths, and for each
    materialised row the plan row it is a copy of"""
    trunk_len = np.asarray(trunk_len, np.int64)
    own_len = np.asarray(own_len, np.int64)
    B, K = own_len.shape
    toff, ooff, _ = plan_layout(trunk_len, own_len)
    src, lens = [], []
    for b in range(B):
        t = np.arange(toff[b], toff[b] + trunk_len[b])
        src.append(t); lens.append(t.size)
        for k in range(K):
            if own_len[b, k]:
                src.append(np.concatenate([t, np.arange(ooff[b, k], ooff[b, k] + own_len[b, k])]))
                lens.append(src[-1].size)
    src = np.concatenate(src) if src else np.zeros(0, np.int64)
    return np.asarray(qkv)[src], [int(n) for n in lens], src


# ---- inputs that are not standard normal: bait keys (a query that sees a key it must not see) and spotlight queries (a query that
# misses a key it must see).  U = head dimension 0 of every head; C = D = 16 is exact in bf16 / fp16 and C * D * 0.125 = 32 puts a
# bait >= 25 above every allowed logit of the data below while |logit| stays under 80 (fp32 exp, fp16 operands).
C_BAIT = 16.0
D_BAIT = 16.0
V_SIGMA = 0.2   # v = 0.2 * standard normal, |v| < 1, in these tests: see rounding_tol


def draw_qkv(rng, rows, heads, v_sigma=1.0):
    x = rng.standard_normal((rows, 3, heads, 64)).astype(np.float32)
    if v_sigma != 1.0:
        x[:, 2] = np.clip(x[:, 2] * v_sigma, -0.96, 0.96)   # 4.8 sigma: outputs stay inside the binade below 1
    return x


def bait(x, trunk_len, own_len, kind):
    """x [rows, 3, heads, 64] (modified in place) -> same: the keys of class `kind` get + C_BAIT along U, their victims'
    queries D_BAIT along U, every other query 0 along U (no row is both bait and victim).
    "next": bait = own keys of odd candidates, victims = queries of even candidates;
    "future": bait = the last own key of every candidate with >= 2 own rows, victims = its earlier queries;
    "other": bait = trunk keys of image 1, victims = branch and trunk queries of every other image."""
    img, cand, pos = plan_rows(trunk_len, own_len)
    own_len = np.asarray(own_len)
    x[:, 0, :, 0] = 0.0
    if kind == "next":
        baits = (cand >= 0) & (cand % 2 == 1)
        victims = (cand >= 0) & (cand % 2 == 0)
    elif kind == "future":
        ln = np.where(cand >= 0, own_len[img, np.maximum(cand, 0)], 0)
        baits = (cand >= 0) & (ln >= 2) & (pos == ln - 1)
        victims = (cand >= 0) & (ln >= 2) & (pos < ln - 1)
    elif kind == "other":
        baits = (cand < 0) & (img == 1)
        victims = img != 1
    else:
        raise ValueError(kind)
    x[baits, 1, :, 0] += C_BAIT
    x[victims, 0, :, 0] = D_BAIT
    return x


SPOT_KINDS = ("trunk0", "trunk_last", "own0", "diag")
SPOT_LOGIT = 40.0   # logit of the target key; another key k' gets 40 cos(k, k'), and cos ~ N(0, 1/64) stays under 0.75


def spotlight(x, trunk_len, own_len, kind):
    """x [rows, 3, heads, 64] (modified in place): every key scaled to |k| = 8 (the norm a standard-normal key has on
    average) and every query aligned with ONE allowed boundary key of its own, q = 5 k_target, so that the target's logit
    is 40 at scale 0.125 and it carries > 0.99 of the weight:
      "trunk0"     trunk key 0                       (a trunk query, or a branch without a trunk: its first key)
      "trunk_last" the last trunk key                (a trunk query, or a branch without a trunk: its diagonal key)
      "own0"       own key 0                         (a trunk query: its first key)
      "diag"       the diagonal key, the query's own row
    -> x, target [rows] (index in the query's key list: trunk keys, then own keys), target_row [rows] (plan row of that key)"""
    trunk_len = np.asarray(trunk_len, np.int64)
    own_len = np.asarray(own_len, np.int64)
    toff, ooff, rows = plan_layout(trunk_len, own_len)
    img, cand, pos = plan_rows(trunk_len, own_len)
    p = trunk_len[img]
    branch = cand >= 0
    own0_row = np.where(branch, ooff[img, np.maximum(cand, 0)], toff[img])
    me = np.arange(rows)
    has_trunk = branch & (p > 0)
    if kind == "trunk0":        # trunk queries: their key 0; branch queries without a trunk: own key 0
        tgt = np.zeros(rows, np.int64)
        trow = np.where(has_trunk, toff[img], own0_row)
    elif kind == "trunk_last":  # trunk queries and branches without a trunk: the diagonal
        tgt = np.where(has_trunk, p - 1, pos)
        trow = np.where(has_trunk, toff[img] + p - 1, me)
    elif kind == "own0":
        tgt = np.where(has_trunk, p, 0)
        trow = own0_row
    elif kind == "diag":
        tgt = np.where(has_trunk, p + pos, pos)
        trow = me
    else:
        raise ValueError(kind)
    x[:, 1] *= 8.0 / np.linalg.norm(x[:, 1], axis=-1, keepdims=True)
    x[:, 0] = (SPOT_LOGIT / 8.0) * x[trow, 1]
    return x, tgt, trow


def _tol_from_model(prec, model, ref, xr, heads):
    """the rule of rounding_tol / seg_rounding_tol: 4 * max |model - ref| + 2 ulp * max |v|, floored for f32 / split-fp16"""
    xr = np.asarray(xr).reshape(-1, 3, heads, 64)
    merr = float(np.abs(model - ref).max()) if ref.size else 0.0
    vmax = float(np.abs(xr[:, 2]).max()) if xr.size else 0.0
    tol = 4.0 * merr + 2.0 * ULP[prec] * vmax
    if prec in (F32, SPLIT):
        tol = max(tol, NORMAL_TOL[prec])
    return tol, merr


def rounding_tol(prec, xr, trunk_len, own_len, heads, scale, ref):
    """Tolerance where the inputs are not standard normal, as a margin over a ROUNDING MODEL OF THE REFERENCE (never over a
    kernel): tol = 4 * max |model - ref| + 2 ulp(output type) * max |v|, floored for f32 / split-fp16 (whose model lies below
    their fp32 accumulation noise) at the bound of the precision on standard-normal data.  The factor 4 covers what the model
    leaves out: per-tile handling of the running maximum, fp32 accumulation order, the hardware exp.
    bf16 / fp16: must stay within twice the standard-normal bound, otherwise the construction is too extreme.  With unit-variance
    v (max |v| ~ 4.5 over a plan) the ulp term alone is 2 * 2^-8 * 4.5 = 3.5e-2 in bf16 and 4.4e-3 in fp16, above those caps
    (3e-2, 4e-3), and a segment of one row returns v itself, so the model error is the output rounding of the largest |v|:
    half a spacing, which doubles at every power of two.  These tests therefore draw v = V_SIGMA * standard normal with
    |v| < 1: both terms scale with v, and so does the effect of a leaked or dropped key (about max |v|), which keeps the
    mutants of test_attn_ref_cpu.py >= 50 tolerances away (4 * 2^-9 + 2 * 2^-8 = 1/64 of max |v| in bf16).
    -> tol, model error"""
    xr = np.asarray(xr).reshape(-1, 3, heads, 64)
    model = plan_ref(xr.reshape(xr.shape[0], -1), trunk_len, own_len, heads, scale, model=prec)
    return _tol_from_model(prec, model, ref, xr, heads)


# ---- plain segments (no prefix), both mask modes: what launch_attention serves for the BERT and vision towers ------------------
def seg_rows(lens):
    """per packed row of plain segments: segment, position inside it, the segment's length"""
    lens = np.asarray(lens, np.int64).reshape(-1)
    seg = np.repeat(np.arange(lens.size), lens)
    pos = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    return seg, pos, lens[seg]


def seg_ref(qkv, lens, heads, causal, scale, mutant=None, model=None, want_weight=None):
    """fp64 context rows [rows, heads*64] of plain segments packed back to back, from operands already rounded to the operand
    type: query i of a segment sees its keys 0..i (causal) or all of them.

    mutant: None, or a reference that is wrong by exactly ONE key: "next" -- every query also sees the row that follows its
    segment (key 0 of the following segment; the last segment has none); "prev" -- every query also sees the row in front of
    its segment (the last key of the preceding segment); "dup_last" -- the last visible key of every query is counted twice
    (what an unmasked padding lane does: those lanes re-read the clamped last key).
    model: None, or a precision code: the rounding model of plan_ref.
    want_weight: None, or [rows] / [rows, 2] key indices inside the query's segment: also returns the softmax weight
    [rows, heads] each query puts on that key, or on the pair (a pair of equal indices counts once)."""
    lens = np.asarray(lens, np.int64).reshape(-1)
    rows = int(lens.sum())
    x = np.ascontiguousarray(qkv, np.float64).reshape(rows, 3, heads, 64)
    out = np.zeros((rows, heads, 64), np.float64)
    wout = np.zeros((rows, heads), np.float64) if want_weight is not None else None
    if want_weight is not None:
        want_weight = np.asarray(want_weight, np.int64).reshape(rows, -1)
    start = np.cumsum(lens) - lens
    for L in np.unique(lens[lens > 0]):   # the segments of one length in one batch
        L = int(L)
        o = start[lens == L]                                     # [S]
        idx = o[:, None] + np.arange(L)[None]                    # [S, L] packed rows
        q, k, v = (x[idx][:, :, c].transpose(0, 2, 1, 3) for c in range(3))   # [S, h, L, d]
        mask = np.tril(np.ones((L, L), bool)) if causal else np.ones((L, L), bool)
        mask = np.broadcast_to(mask, (o.size, 1, L, L))
        if mutant in ("next", "prev"):
            er = o + L if mutant == "next" else o - 1
            has = (er >= 0) & (er < rows)
            er = np.clip(er, 0, rows - 1)
            k = np.concatenate([k, x[er, 1][:, :, None]], 2)
            v = np.concatenate([v, x[er, 2][:, :, None]], 2)
            mask = np.concatenate([mask, np.broadcast_to(has[:, None, None, None], (o.size, 1, L, 1))], 3)
        s = np.matmul(q, k.transpose(0, 1, 3, 2)) * scale       # [S, h, L, M]
        s = np.where(mask, s, -np.inf)
        e = np.exp(s - s.max(-1, keepdims=True))
        if mutant == "dup_last":
            last = np.arange(L) if causal else np.full(L, L - 1)
            e[:, :, np.arange(L), last] *= 2.0
        den = e.sum(-1, keepdims=True)
        if wout is not None:
            t = want_weight[idx]                                 # [S, L, 1 or 2]
            hit = (np.arange(k.shape[2])[None, None, None] == t[..., None]).any(2)   # [S, L, M]
            wout[idx] = ((e / den) * hit[:, None]).sum(-1).transpose(0, 2, 1)
        if model is not None:
            e = _round64(model, e)
        ctx = (np.matmul(e, v) / den).transpose(0, 2, 1, 3)      # [S, L, h, d]
        out[idx] = _round64(model, ctx) if model is not None else ctx
    out = out.reshape(rows, heads * 64)
    return (out, wout) if want_weight is not None else out


def seg_rounding_tol(prec, xr, lens, heads, causal, scale, ref):
    """rounding_tol for plain segments: the same rule over seg_ref's rounding model.  -> tol, model error"""
    xr = np.asarray(xr).reshape(-1, 3, heads, 64)
    model = seg_ref(xr.reshape(xr.shape[0], -1), lens, heads, causal, scale, model=prec)
    return _tol_from_model(prec, model, ref, xr, heads)


def seg_bait(x, lens, parity):
    """x [rows, 3, heads, 64] (modified in place) -> same.  The segments that have rows are numbered in memory order; the keys
    of those of `parity` (0 / 1) get + C_BAIT along U, the queries of the others D_BAIT along it, every other query 0 along it:
    the rows on either side of a victim segment are bait, and no row is both.  Run both parities: every segment with a
    neighbour is a victim once.  v is clipped to 3.5 V_SIGMA: a context row is a convex combination of v rows (and row 0 of a
    causal segment IS a v row), so the true reference stays under 4 V_SIGMA by construction, not by the luck of a seed."""
    seg, _, _ = seg_rows(lens)
    np.clip(x[:, 2], -3.5 * V_SIGMA, 3.5 * V_SIGMA, out=x[:, 2])
    lens = np.asarray(lens, np.int64).reshape(-1)
    ordinal = np.cumsum(lens > 0) - 1          # number of the segment among those that have rows
    baits = ordinal[seg] % 2 == parity
    x[:, 0, :, 0] = 0.0
    x[baits, 1, :, 0] += C_BAIT
    x[~baits, 0, :, 0] = D_BAIT
    return x


def seg_victims(lens, parity, mutant):
    """rows of seg_bait(parity) whose output a "next" / "prev" mutant must move: victim queries with such a neighbour"""
    seg, _, ln = seg_rows(lens)
    lens = np.asarray(lens, np.int64).reshape(-1)
    ordinal = np.cumsum(lens > 0) - 1
    start = np.repeat(np.cumsum(lens) - lens, lens)
    has = start + ln < int(lens.sum()) if mutant == "next" else start > 0
    return (ordinal[seg] % 2 != parity) & has


SEG_SPOT_KINDS = ("key0", "last", "key31", "key32", "key63", "key64", "diag")


def _seg_last_visible(lens, causal):
    _, pos, ln = seg_rows(lens)
    return pos if causal else ln - 1


def seg_spotlight(x, lens, kind, causal):
    """spotlight() for plain segments: every key scaled to |k| = 8 and q = 5 k_target (logit SPOT_LOGIT at scale 0.125), the
    target being key 0, the last visible key (the diagonal under the causal mask, the segment's last key otherwise), the key
    at 31 / 32 / 63 / 64 -- either side of a 32-key tile edge -- clamped to the last visible key, or the diagonal.
    -> x, target [rows] (key index inside the segment), target_row [rows] (packed row of that key)"""
    seg, pos, ln = seg_rows(lens)
    lastv = _seg_last_visible(lens, causal)
    if kind == "key0":
        tgt = np.zeros_like(pos)
    elif kind == "last":
        tgt = lastv
    elif kind == "diag":
        tgt = pos
    elif kind in SEG_SPOT_KINDS:
        tgt = np.minimum(int(kind[3:]), lastv)
    else:
        raise ValueError(kind)
    trow = np.arange(pos.size) - pos + tgt
    x[:, 1] *= 8.0 / np.linalg.norm(x[:, 1], axis=-1, keepdims=True)
    x[:, 0] = (SPOT_LOGIT / 8.0) * x[trow, 1]
    return x, tgt, trow


def seg_twin(x, lens, causal):
    """every key scaled to |k| = 8 and q = 5 (k_0 + k_last) / (1 + cos(k_0, k_last)), k_last the last visible key: key 0 and the
    last visible key carry logit SPOT_LOGIT each and share the weight, so a last key counted twice moves the row by a sixth of
    v_last - v_0.  Where the two are one key (a segment of one row, query 0 under the causal mask) this is a spotlight.
    -> x, pair [rows, 2] (key indices inside the segment)"""
    seg, pos, ln = seg_rows(lens)
    lastv = _seg_last_visible(lens, causal)
    me = np.arange(pos.size)
    r0, r1 = me - pos, me - pos + lastv
    x[:, 1] *= 8.0 / np.linalg.norm(x[:, 1], axis=-1, keepdims=True)
    k0, k1 = x[r0, 1], x[r1, 1]
    cos = (k0 * k1).sum(-1, keepdims=True) / 64.0
    x[:, 0] = (SPOT_LOGIT / 8.0) * (k0 + k1) / (1.0 + cos)
    return x, np.stack([np.zeros_like(pos), lastv], 1)
