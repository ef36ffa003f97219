"""ctypes wrappers of the hooks behind the text tower's first- and last-layer reductions (include/conzic_hip_test.h):
czc_test_attention_pooled / czc_test_attention_mapped (attention_image_kernel's pooled and mapped modes, one launch on a
host-given plan) and czc_test_layer0_plan (the plan chain with the distinct-row plan of layer 0), czc_test_text_tower (an engine's text tower on
host-given CLIP id rows).  TEST INFRASTRUCTURE, beside
tests/kernel_hooks.py (same guards, same sentinels)."""
import ctypes as C

import numpy as np

from conzic_amd import native
from kernel_hooks import GUARD, PLAN_GUARD


def attention_pooled(prec, trunk_len, own_len, rep, heads, scale, qkv, qc):
    """trunk_len [B], own_len [B, K], rep [B, K] (candidate k of image b rides on candidate rep[b, k], itself where it has rows), qkv fp32 [rows, 3*heads*64] (k / v are
    read), qc fp32 [B*K, heads*64] (one q row per candidate).  -> (ctx [B*K, heads*64], guard [2*PLAN_GUARD, heads*64])."""
    lib = native.load_test()
    tl = np.ascontiguousarray(trunk_len, np.int32)
    ol = np.ascontiguousarray(own_len, np.int32)
    B, K = ol.shape
    assert tl.shape == (B,)
    rows = int(tl.sum()) + int(ol.sum())
    pi = np.ascontiguousarray(rep, np.int32).reshape(B * K)
    qkv = np.ascontiguousarray(qkv, np.float32).reshape(rows, 3 * heads * 64)
    qc = np.ascontiguousarray(qc, np.float32).reshape(B * K, heads * 64)
    full = np.empty((B * K + 2 * PLAN_GUARD, heads * 64), np.float32)
    rc = lib.czc_test_attention_pooled(int(prec), B, K, int(heads), C.c_float(scale), tl.ctypes.data, ol.ctypes.data, pi.ctypes.data,
                                       qkv.ctypes.data, qc.ctypes.data, full.ctypes.data)
    native.check(rc, None, "czc_test_attention_pooled")
    return full[PLAN_GUARD:PLAN_GUARD + B * K], np.concatenate([full[:PLAN_GUARD], full[PLAN_GUARD + B * K:]])


def attention_mapped(prec, trunk_len, own_len, rowmap, heads, scale, qkv):
    """qkv fp32 [n_rows, 3*heads*64] holds packed row r of the plan at row rowmap[r].  -> (out [rows, heads*64], guard)."""
    lib = native.load_test()
    tl = np.ascontiguousarray(trunk_len, np.int32)
    ol = np.ascontiguousarray(own_len, np.int32)
    B, K = ol.shape
    rows = int(tl.sum()) + int(ol.sum())
    rm = np.ascontiguousarray(rowmap, np.int32).reshape(rows)
    qkv = np.ascontiguousarray(qkv, np.float32)
    n_rows = qkv.shape[0]
    assert qkv.shape == (n_rows, 3 * heads * 64)
    full = np.empty((rows + 2 * PLAN_GUARD, heads * 64), np.float32)
    rc = lib.czc_test_attention_mapped(int(prec), B, K, int(heads), C.c_float(scale), tl.ctypes.data, ol.ctypes.data, rm.ctypes.data,
                                       n_rows, qkv.ctypes.data, full.ctypes.data)
    native.check(rc, None, "czc_test_attention_mapped")
    return full[PLAN_GUARD:PLAN_GUARD + rows], np.concatenate([full[:PLAN_GUARD], full[PLAN_GUARD + rows:]])


def layer0_plan(ids, length, dedup=True):
    """ids [B, K, 77], length [B, K] -> dict(own_off [S + 1], own_len [S], dcount [B], totals [12], rowmap [M], dist [D]) with
    .guards checked (two calls of the hook: the sizes first, as the engine reads them back, then the map)."""
    lib = native.load_test()
    ids = np.ascontiguousarray(ids, np.int32)
    ln = np.ascontiguousarray(length, np.int32)
    B, K = ln.shape
    S = B + B * K

    def call(M, D):
        bufs = {n: np.zeros(w + 2 * GUARD, np.int32) for n, w in
                (("own_off", S + 1), ("own_len", S), ("dcount", B), ("totals", 12), ("rowmap", max(M, 1)), ("dist", max(D, 1)))}
        rc = lib.czc_test_layer0_plan(B, K, ids.ctypes.data, ln.ctypes.data, 1 if dedup else 0, bufs["own_off"].ctypes.data,
                                      bufs["own_len"].ctypes.data, bufs["dcount"].ctypes.data, bufs["totals"].ctypes.data, M,
                                      bufs["rowmap"].ctypes.data, D, bufs["dist"].ctypes.data)
        native.check(rc, None, "czc_test_layer0_plan")
        out = {}
        for n, full in bufs.items():
            g = np.concatenate([full[:GUARD], full[full.size - GUARD:]])
            assert (g == 0x5A5A5A5A).all(), f"{n}: stray store into the guard words"
            out[n] = full[GUARD:full.size - GUARD]
        return out

    first = call(0, 0)
    M, D = int(first["totals"][0]), int(first["totals"][6] + first["totals"][8])
    res = call(M, D)
    for n in ("own_off", "own_len", "dcount", "totals"):
        assert (res[n] == first[n]).all(), n
    return res


def text_tower(engine, ids, length):
    """The text tower of `engine` on ids [B, K, 77] / length [B, K] through the step's own plan -> (features [B*K, proj], number
    of candidates that ride on an identical one)."""
    lib = native.load_test()
    ids = np.ascontiguousarray(ids, np.int32)
    ln = np.ascontiguousarray(length, np.int32)
    B, K = ln.shape
    assert ids.shape == (B, K, native.CLIP_MAX_LEN)
    feat = np.empty((B * K, engine.clip_cfg.proj), np.float32)
    n_dup = C.c_int32(-1)
    rc = lib.czc_test_text_tower(engine.h, B, K, ids.ctypes.data, ln.ctypes.data, feat.ctypes.data, C.addressof(n_dup))
    native.check(rc, None, "czc_test_text_tower")
    return feat, int(n_dup.value)
