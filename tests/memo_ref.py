"""numpy models of the integer kernels of csrc/rowops.hip (gathers, masks, tied rows), csrc/memo.hip and csrc/memo_rows.hip, and the
inputs the CPU and GPU tests share.  Every model states the operation word for word: buffers a chain may write start as the input (or as
the hooks' pre-fill pattern SENT where the chain only writes them) and are compared with the device's whole buffers bit for bit."""
import numpy as np

SENT = 0x5A5A5A5A       # bytes 0x5a: what a word no kernel wrote holds (tests/kernel_hooks.py SENTINEL)
POS_IDLE = -1           # include/conzic_hip.h CZC_POS_IDLE
SUB = 2                 # csrc/kernels.h MEMO_ROWS_SUB
MISS, HIT, IDLE = 0, 1, 2
MASK_ID = 3


def sent(shape, dtype=np.int32):
    return np.full(shape, SENT, np.uint32).view(dtype)


def same_words(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.size == b.size and np.array_equal(a.reshape(-1).view(np.uint32), b.reshape(-1).view(np.uint32))


# ---- movers -----------------------------------------------------------------------------------------------------------------------
def gather_rows(src, idx):
    return np.asarray(src)[np.asarray(idx)]


def masked(rows, col, n_mask, mask_id):
    """rows [N, T] with columns col .. col + n_mask - 1 (inside the row) set to mask_id; col a scalar or [N]"""
    rows = np.array(rows, np.int32, copy=True)
    N, T = rows.shape
    c = np.broadcast_to(np.asarray(col), (N,))[:, None]
    t = np.arange(T)[None, :]
    rows[(t >= c) & (t < c + n_mask)] = mask_id
    return rows


def mask_positions(inp, gen, n_mask, mask_id):
    """launch_mask_positions (gen scalar) / launch_mask_positions_rows (gen [B]; a row with gen < 0 is left alone)"""
    inp = np.asarray(inp, np.int32)
    if np.isscalar(gen):
        return masked(inp, gen, n_mask, mask_id)
    g = np.asarray(gen)
    out = masked(inp, np.where(g >= 0, g, inp.shape[1]), n_mask, mask_id)
    return out


def tie_rows(inp, col, grp_of_row, grp_off, grp_rows):
    """every row r that ran at a column 0 <= c < T copies inp[r, c] into column c of the other members of its group.  Defined only
    where the members of a group run at distinct columns (tie_inputs_ok)."""
    src = np.asarray(inp, np.int32)
    out = src.copy()
    R, T = src.shape
    for r in range(R):
        c = int(col[r])
        if c < 0 or c >= T:
            continue
        g = int(grp_of_row[r])
        for m in grp_rows[grp_off[g]:grp_off[g + 1]]:
            if m != r and 0 <= m < R:
                out[m, c] = src[r, c]
    return out


def tie_inputs_ok(col, grp_off, grp_rows, T):
    for g in range(len(grp_off) - 1):
        cs = [int(col[m]) for m in grp_rows[grp_off[g]:grp_off[g + 1]] if 0 <= int(col[m]) < T]
        if len(cs) != len(set(cs)):
            return False
    return True


# ---- image memo (memo.hip) ---------------------------------------------------------------------------------------------------------
MEMO_PATTERNS = ("all_hit", "all_miss", "alternating", "chunk_last", "random", "last_column", "in_window")


def memo_state(B, T, D, gen_idx, n_mask, pattern, seed=0):
    """Inputs of the image memo chain: the batch, the stored keys by `pattern`, the entry of the sub-step, what the step would leave."""
    rng = np.random.default_rng(seed + 7 * B + n_mask)
    inp = rng.integers(5, 1000, (B, T)).astype(np.int32)
    key = masked(inp, gen_idx, n_mask, MASK_ID)
    b = np.arange(B)
    miss = {"all_hit": b < 0, "all_miss": b >= 0, "alternating": b % 2 == 1, "chunk_last": (b % 256 == 255) | (b == B - 1),
            "random": rng.random(B) < 0.4, "last_column": b % 2 == 0, "in_window": b < 0}[pattern]
    free = [t for t in range(T) if not (gen_idx <= t < gen_idx + n_mask)]
    for i in np.nonzero(miss)[0]:
        t = T - 1 if pattern == "last_column" else free[int(rng.integers(len(free)))]
        if pattern == "last_column" and t not in free:
            t = free[-1]
        key[i, t] += 1
    if pattern == "in_window":  # the batch differs from what the key's visit saw, but only where the mask goes
        inp[:, gen_idx:gen_idx + n_mask] = 7
    return dict(inp=inp, key=key, img_max=rng.integers(1, 30, (2, B)).astype(np.int32),
                img_n=rng.standard_normal((B, D)).astype(np.float32), new_rows=rng.integers(5, 1000, (B, T)).astype(np.int32),
                new_cos=rng.random(B).astype(np.float32), new_max=rng.integers(1, 30, B).astype(np.int32),
                ent_rows=rng.integers(5, 1000, (B, T)).astype(np.int32), ent_cos=rng.random(B).astype(np.float32),
                ent_max=rng.integers(1, 30, B).astype(np.int32), bcos=rng.random(B).astype(np.float32), miss=miss)


def memo_chain(st, gen_idx, n_mask, mask_id, n_sub, stages=1, use_list=1, record=1):
    """launch_memo_check [-> fill -> gather -> the step -> scatter], as czc_test_memo_chain chains them -> every buffer"""
    inp, key = st["inp"].copy(), st["key"].copy()
    B, T = inp.shape
    D = st["img_n"].shape[1]
    same = (masked(inp, gen_idx, n_mask, mask_id) == key).all(1)
    lst = np.nonzero(~same)[0]
    n = len(lst)
    o = dict(hit=same.astype(np.int32), list=sent(B), tot=np.zeros(4, np.int32), key=key, inp=inp, bcos=st["bcos"].copy(),
             ent_rows=st["ent_rows"].copy(), ent_cos=st["ent_cos"].copy(), ent_max=st["ent_max"].copy(), inp_c=sent((B, T)),
             img_c=sent((B, D), np.float32))
    o["list"][:n] = lst
    o["tot"][0] = n
    for j in range(min(n_sub, 2)):
        o["tot"][1 + j] = max(0, int(st["img_max"][j][same].max())) if same.any() else 0
    if not stages:
        return o
    if n < B:  # fill: the hit images take the entry's row and cosine
        o["inp"][same] = o["ent_rows"][same]
        o["bcos"][same] = o["ent_cos"][same]
    if n == 0:
        return o
    run = lst if use_list else np.arange(B)
    if record:
        o["key"][run] = masked(o["inp"][run], gen_idx, n_mask, mask_id)
    if use_list:
        o["inp_c"][:n] = o["inp"][run]
        o["img_c"][:n] = st["img_n"][run]
        o["inp"][run] = st["new_rows"][run]
    o["bcos"][run] = st["new_cos"][run]
    if record:
        o["ent_rows"][run] = st["new_rows"][run]
        o["ent_cos"][run] = st["new_cos"][run]
        o["ent_max"][run] = st["new_max"][run]
    return o


# ---- rows memo (memo_rows.hip) -----------------------------------------------------------------------------------------------------
ROWS_PATTERNS = MEMO_PATTERNS + ("mixed",)


def rows_sig(n_mask0, n_sub, col1, R):
    """the signature word of a group per row [R]: n_mask | length << 8 | (column of the second step + 1) << 16"""
    c1 = np.asarray(col1, np.int64) + 1 if (n_sub > 1 and col1 is not None) else np.zeros(R, np.int64)
    return ((n_mask0 & 0xFF) | (n_sub << 8) | (c1 << 16)).astype(np.int32)


def rows_pos(col0, seed_len, L):
    p = np.asarray(col0, np.int64) - seed_len
    return np.where((np.asarray(col0) >= 0) & (p >= 0) & (p < L), p, -1)


def rows_state(R, T, L, seed_len, D, n_mask0, n_sub, pattern, with_col1=True, seed=0):
    """Inputs of the rows memo chain.  Every row visits its own column; the table holds, by `pattern`, a matching entry or one that
    differs somewhere.  "mixed" adds what only the rows form has: idle rows, valid == 0, each signature field differing, drawing rows
    (tau > 0), columns outside [seed_len, seed_len + L), and imax <= 0 in hit slots."""
    rng = np.random.default_rng(seed + 13 * R + n_mask0 + 100 * n_sub)
    inp = rng.integers(5, 1000, (R, T)).astype(np.int32)
    col0 = (seed_len + rng.integers(0, L, R)).astype(np.int32)
    col1 = (seed_len + rng.integers(0, L, R)).astype(np.int32) if (with_col1 and n_sub > 1) else None
    r = np.arange(R)
    valid = np.ones((L, R), np.int32)
    sig = np.broadcast_to(rows_sig(n_mask0, n_sub, col1, R), (L, R)).copy()
    key = np.broadcast_to(masked(inp, col0, n_mask0, MASK_ID), (L, R, T)).copy()
    tau = None
    base = pattern if pattern != "mixed" else "random"
    miss = {"all_hit": r < 0, "all_miss": r >= 0, "alternating": r % 2 == 1, "chunk_last": (r % 256 == 255) | (r == R - 1),
            "random": rng.random(R) < 0.4, "last_column": r % 2 == 0, "in_window": r < 0}[base]
    for i in np.nonzero(miss)[0]:
        c = int(col0[i])
        free = [t for t in range(T) if not (c <= t < c + n_mask0)]
        t = free[-1] if base == "last_column" else free[int(rng.integers(len(free)))]
        key[:, i, t] += 1
    if base == "in_window":
        for i in range(R):
            inp[i, col0[i]:col0[i] + n_mask0] = 7
    imax = rng.integers(1, 30, (L, SUB, R)).astype(np.int32)
    if pattern == "mixed":
        kind = rng.integers(0, 10, R)
        col0[kind == 0] = POS_IDLE                                   # sits the group out
        valid[:, kind == 1] = 0                                      # never recorded
        sig[:, kind == 2] ^= 1                                       # another n_mask
        sig[:, kind == 3] ^= 1 << 8                                  # another group length
        sig[:, kind == 4] ^= 1 << 16                                 # another second column
        tau = np.where(kind == 5, 0.7, 0.0).astype(np.float32)       # draws its winner: never a hit
        col0[kind == 6] = seed_len + L + (r[kind == 6] % 3)          # column behind the caption: a miss, no slot
        col0[(kind == 6) & (r % 2 == 0) & (seed_len > 0)] = seed_len - 1   # ... or in front of it
        imax[:, :, kind == 7] = -rng.integers(0, 5, (L, SUB, int((kind == 7).sum())))  # imax <= 0 is ignored
    return dict(inp=inp, col0=col0, col1=col1, tau=tau, col=rng.integers(0, T, R).astype(np.int32), dot=rng.integers(0, 2, R).astype(np.int32),
                img_n=rng.standard_normal((R, D)).astype(np.float32), new_rows=rng.integers(5, 1000, (R, T)).astype(np.int32),
                new_cos=rng.random(R).astype(np.float32), new_max=rng.integers(1, 30, R).astype(np.int32),
                bcos=rng.random(R).astype(np.float32), valid=valid, sig=sig, key=key,
                rows=rng.integers(5, 1000, (L, SUB, R, T)).astype(np.int32), cos=rng.random((L, SUB, R)).astype(np.float32), imax=imax)


def rows_chain(st, L, seed_len, n_mask0, n_sub, mask_id, j=0, stages=1, use_list=1, record=1):
    """launch_memo_rows_check [-> fill -> gather -> the step -> scatter], as czc_test_memo_rows_chain chains them -> every buffer"""
    inp = st["inp"].copy()
    R, T = inp.shape
    D = st["img_n"].shape[1]
    col0 = st["col0"]
    p = rows_pos(col0, seed_len, L)
    idle = col0 < 0
    sg = rows_sig(n_mask0, n_sub, st["col1"], R)
    rr = np.arange(R)
    ps = np.maximum(p, 0)
    o = dict(valid=st["valid"].copy(), sig=st["sig"].copy(), key=st["key"].copy(), rows=st["rows"].copy(), cos=st["cos"].copy(),
             imax=st["imax"].copy(), list=sent(R), tot=np.zeros(4, np.int32), inp=inp, bcos=st["bcos"].copy(), inp_c=sent((R, T)),
             img_c=sent((R, D), np.float32), col_c=sent(R), dot_c=sent(R))
    same = (p >= 0) & (o["valid"][ps, rr] == 1) & (o["sig"][ps, rr] == sg)
    if st["tau"] is not None:
        same &= ~(st["tau"] > 0)
    same &= (masked(inp, col0, n_mask0, mask_id) == o["key"][ps, rr]).all(1)
    hit = np.where(idle, IDLE, np.where(same, HIT, MISS)).astype(np.int32)
    lst = np.nonzero(hit == MISS)[0]
    n = len(lst)
    o["hit"] = hit
    o["cnt"] = np.array([int((hit[g:g + 256] == MISS).sum()) for g in range(0, R, 256)], np.int32)
    o["list"][:n] = lst
    o["tot"][0] = n
    for s in range(min(n_sub, SUB)):
        v = o["imax"][ps, s, rr][same]
        o["tot"][1 + s] = max(0, int(v.max())) if v.size else 0
    if not stages:
        return o
    if n < R:  # fill: the hit rows take sub-step j of their slot back
        h = hit == HIT
        o["inp"][h] = o["rows"][ps[h], j, rr[h]]
        o["bcos"][h] = o["cos"][ps[h], j, rr[h]]
    if n == 0:
        return o
    run = lst if use_list else rr
    rec = run[p[run] >= 0] if record else run[:0]
    o["key"][p[rec], rec] = masked(o["inp"][rec], col0[rec], n_mask0, mask_id)
    o["valid"][p[rec], rec] = 1
    o["sig"][p[rec], rec] = sg[rec]
    if use_list:
        o["inp_c"][:n] = o["inp"][run]
        o["img_c"][:n] = st["img_n"][run]
        o["col_c"][:n] = st["col"][run]
        o["dot_c"][:n] = st["dot"][run]
        o["inp"][run] = st["new_rows"][run]
    o["bcos"][run] = st["new_cos"][run]
    o["rows"][p[rec], j, rec] = st["new_rows"][rec]
    o["cos"][p[rec], j, rec] = st["new_cos"][rec]
    o["imax"][p[rec], j, rec] = st["new_max"][rec]
    return o
