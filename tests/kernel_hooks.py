"""Kernel-level hooks for tests/ and tools/: typed numpy wrappers over libconzic_hip_test.so (include/conzic_hip_test.h).

TEST INFRASTRUCTURE.  Each function runs ONE kernel family of the product library on host data so that a `-m gpu` test can
compare it with the CPU oracle; nothing in conzic_amd/ imports this module and the product library exports none of the
symbols behind it.  (Until round 5 these lived in conzic_amd/engine.py as test_*; the names lost the prefix here so that
pytest does not collect them.)

Families with a kernel-level test of their own: GEMM / LayerNorm / attention / top-K / bridge / combine (tests/test_kernels_gpu.py), the
shared-prefix attention plans, the per-sequence attention launches (attention_seq: tests/test_attention_seq_gpu.py), the
selection and plan kernels, the row / embedding / mover / memo kernels, the fluency kernels, the
text bridge with candidates in its three forms (tests/test_bridge_kernel_gpu.py against the string reference tests/bridge_ref.py,
pinned by tests/test_bridge_ref_cpu.py), the per-row forms of the top-K selection (tests/test_topk_rows_gpu.py), the combine kernel in
its scalar, per-row and drawing forms (tests/combine_hooks.py: tests/test_combine_kernel_gpu.py against the fp64 reference and the
derived bars of tests/combine_ref.py, pinned by tests/test_combine_ref_cpu.py), and -- at the end
of this file -- every GEMM family on strided, windowed and in-place buffers (gemm_layout: tests/test_gemm_layout_gpu.py, with the
cases, the fp64 reference and the checker in tests/gemm_layout.py, pinned by tests/test_gemm_layout_cpu.py).

Three kinds of guarded result: the attention-plan hooks return their guard rows beside the rows (PLAN_GUARD, PLAN_SENTINEL);
the integer / row / bridge hooks return a Guarded (GUARD words around every 1-D output, untouched()); gemm_layout returns a
gemm_layout.Launch (whole 2-D output buffers, guard rows and pad columns included) plus the kernel family the launcher chose.
"""
import contextlib
import ctypes as C

import numpy as np

from conzic_amd import native
from conzic_amd.bridge import BridgeArrays
from conzic_amd.engine import _ptr


def gemm(prec, A, W, bias=None, resid=None, act=0, typed_out=False):
    lib = native.load_test()
    if typed_out:
        act |= 0x100
    A = np.ascontiguousarray(A, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    M, K = A.shape
    N = W.shape[0]
    Cm = np.empty((M, N), np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    r = None if resid is None else np.ascontiguousarray(resid, np.float32)
    native.check(lib.czc_test_gemm(prec, M, N, K, A.ctypes.data, W.ctypes.data, _ptr(b), _ptr(r), act, Cm.ctypes.data),
                 None, "czc_test_gemm")
    return Cm


def ln_fold_gemm(prec, x, W, gamma, beta, bias, part, eps, act=0, want_rowsum=False):
    """act(LN(fp16(x)) . W^T + bias) through the folded-LayerNorm weight-stationary GEMM; part [16, M, 2] = partials of fp16(x).
    want_rowsum: also the sums of the stored (centred, fp16) weight rows."""
    lib = native.load_test()
    x = np.ascontiguousarray(x, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    M, N = x.shape[0], W.shape[0]
    g = np.ascontiguousarray(gamma, np.float32)
    bt = np.ascontiguousarray(beta, np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    pt = np.ascontiguousarray(part, np.float32)
    assert pt.shape == (16, M, 2) and x.shape[1] == 512 and W.shape[1] == 512
    out = np.empty((M, N), np.float32)
    rowsum = np.empty(N, np.float32)
    native.check(lib.czc_test_ln_fold_gemm(prec, M, N, x.ctypes.data, W.ctypes.data, g.ctypes.data, bt.ctypes.data, _ptr(b), pt.ctypes.data,
                                           float(eps), int(act), out.ctypes.data, rowsum.ctypes.data), None, "czc_test_ln_fold_gemm")
    return (out, rowsum) if want_rowsum else out


def gemm_x16(prec, A, W, bias, resid, want_part=False):
    """x = fp16(fp16(resid) + A.W^T + bias) on a 2-byte residual stream (GemmArgs::x16); returned as fp32
    (with want_part: also the LayerNorm partials [N/32, M, 2])."""
    lib = native.load_test()
    A = np.ascontiguousarray(A, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    M, K = A.shape
    N = W.shape[0]
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    r = np.ascontiguousarray(resid, np.float32)
    out = np.empty((M, N), np.float32)
    part = np.empty((N // 32, M, 2), np.float32) if want_part else None
    native.check(lib.czc_test_gemm_x16(prec, M, N, K, A.ctypes.data, W.ctypes.data, _ptr(b), r.ctypes.data, out.ctypes.data, _ptr(part)),
                 None, "czc_test_gemm_x16")
    return (out, part) if want_part else out


def layernorm_x16(prec, x, gamma, beta, eps):
    lib = native.load_test()
    x = np.ascontiguousarray(x, np.float32)
    M = x.shape[0]
    assert x.shape[1] == 512
    g = np.ascontiguousarray(gamma, np.float32)
    b = np.ascontiguousarray(beta, np.float32)
    y = np.empty_like(x)
    native.check(lib.czc_test_layernorm_x16(prec, M, x.ctypes.data, g.ctypes.data, b.ctypes.data, float(eps), y.ctypes.data),
                 None, "czc_test_layernorm_x16")
    return y


def gemm_rowln(prec, A, W, bias, resid, gamma, beta, eps):
    """x = resid + A.W^T + bias and y = LayerNorm(x) from the full-row kernel (W has 512 rows)."""
    lib = native.load_test()
    A = np.ascontiguousarray(A, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    M, K = A.shape
    assert W.shape == (512, K)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    r = np.ascontiguousarray(resid, np.float32)
    g = np.ascontiguousarray(gamma, np.float32)
    bt = np.ascontiguousarray(beta, np.float32)
    x = np.empty((M, 512), np.float32)
    y = np.empty((M, 512), np.float32)
    native.check(lib.czc_test_gemm_rowln(prec, M, K, A.ctypes.data, W.ctypes.data, _ptr(b), r.ctypes.data, g.ctypes.data,
                                         bt.ctypes.data, C.c_float(eps), x.ctypes.data, y.ctypes.data), None,
                 "czc_test_gemm_rowln")
    return x, y


def layernorm(prec, x, gamma, beta, eps):
    lib = native.load_test()
    x = np.ascontiguousarray(x, np.float32)
    g = np.ascontiguousarray(gamma, np.float32)
    b = np.ascontiguousarray(beta, np.float32)
    y = np.empty_like(x)
    native.check(lib.czc_test_layernorm(prec, x.shape[0], x.shape[1], x.ctypes.data, g.ctypes.data, b.ctypes.data,
                                        C.c_float(eps), y.ctypes.data), None, "czc_test_layernorm")
    return y


def attention(prec, qkv, seq_len, heads, causal, scale):
    lib = native.load_test()
    qkv = np.ascontiguousarray(qkv, np.float32)
    sl = np.ascontiguousarray(seq_len, np.int32)
    out = np.empty((qkv.shape[0], heads * 64), np.float32)
    native.check(lib.czc_test_attention(prec, sl.size, sl.ctypes.data, heads, 1 if causal else 0, C.c_float(scale),
                                        qkv.ctypes.data, out.ctypes.data), None, "czc_test_attention")
    return out


PLAN_REFUSED = 100   # include/conzic_hip_test.h CZC_TEST_REFUSED
PLAN_GUARD = 32      # CZC_TEST_PLAN_GUARD: rows in front of and behind the plan rows of the hook's device buffers
# what the output pre-fill (bytes 0x5a) reads back as through each precision's output type
PLAN_SENTINEL = {1: float(np.array([0x5A5A5A5A], np.uint32).view(np.float32)[0]),
                 0: float(np.array([0x5A5A0000], np.uint32).view(np.float32)[0]),
                 4: float(np.array([0x5A5A], np.uint16).view(np.float16)[0]),
                 3: 2.0 * float(np.array([0x5A5A], np.uint16).view(np.float16)[0])}


def attention_plan(prec, kernel, trunk_len, own_len, heads, scale, qkv, img_max=True):
    """One attention launch on a shared-prefix plan (czc_test_attention_plan): kernel 0 generic per-segment kernels in their
    prefix form, 1 packed per-group kernel, 2 packed per-image kernel (forced).  trunk_len [B], own_len [B, K], qkv fp32
    [rows, 3*heads*64].  -> (refused, out [rows, heads*64], guard [2*PLAN_GUARD, heads*64]): `refused` when the packed launcher
    returned -1 (nothing launched); `guard` = the output buffer's rows in front of and behind the plan rows."""
    lib = native.load_test()
    tl = np.ascontiguousarray(trunk_len, np.int32)
    ol = np.ascontiguousarray(own_len, np.int32)
    B, K = ol.shape
    assert tl.shape == (B,)
    rows = int(tl.sum()) + int(ol.sum())
    qkv = np.ascontiguousarray(qkv, np.float32).reshape(rows, 3 * heads * 64)
    full = np.empty((rows + 2 * PLAN_GUARD, heads * 64), np.float32)
    rc = lib.czc_test_attention_plan(int(prec), int(kernel), B, K, int(heads), C.c_float(scale), tl.ctypes.data, ol.ctypes.data,
                                     1 if img_max else 0, qkv.ctypes.data, full.ctypes.data)
    if rc != PLAN_REFUSED:
        native.check(rc, None, "czc_test_attention_plan")
    return rc == PLAN_REFUSED, full[PLAN_GUARD:PLAN_GUARD + rows], np.concatenate([full[:PLAN_GUARD], full[PLAN_GUARD + rows:]])


def attention_seq(prec, qkv, heads, causal, scale, seq_len=None, n_seg=None, fixed_T=0, max_keys=0):
    """One launch_attention call on plain segments (czc_test_attention_seq): seq_len given -> own_off / own_len tables (zero-length
    segments allowed); seq_len None -> the fixed_T form, n_seg segments of fixed_T rows.  max_keys 0: the longest segment.
    qkv fp32 [rows, 3*heads*64].  -> (out [rows, heads*64], guard [2*PLAN_GUARD, heads*64]); the launcher's refusal raises
    native.NativeError with the launcher's message."""
    lib = native.load_test()
    if seq_len is not None:
        sl = np.ascontiguousarray(seq_len, np.int32).reshape(-1)
        n_seg, rows, slp = sl.size, int(sl.sum()), sl.ctypes.data
    else:
        n_seg, rows, slp = int(n_seg), int(n_seg) * int(fixed_T), None
    qkv = np.ascontiguousarray(qkv, np.float32).reshape(rows, 3 * heads * 64)
    full = np.empty((rows + 2 * PLAN_GUARD, heads * 64), np.float32)
    native.check(lib.czc_test_attention_seq(int(prec), n_seg, slp, int(fixed_T), int(max_keys), int(heads), 1 if causal else 0,
                                            C.c_float(scale), qkv.ctypes.data, full.ctypes.data), None, "czc_test_attention_seq")
    return full[PLAN_GUARD:PLAN_GUARD + rows], np.concatenate([full[:PLAN_GUARD], full[PLAN_GUARD + rows:]])


def topk(logits, mask, K, temperature, dot_id, dot_allowed):
    lib = native.load_test()
    lg = np.ascontiguousarray(logits, np.float32)
    mk = np.ascontiguousarray(np.asarray(mask, np.float32).reshape(-1))
    B, V = lg.shape
    p = np.empty((B, K), np.float32)
    i = np.empty((B, K), np.int32)
    c = np.empty((B, K), np.int32)
    native.check(lib.czc_test_topk(B, V, K, lg.ctypes.data, mk.ctypes.data, C.c_float(temperature), dot_id,
                                   1 if dot_allowed else 0, p.ctypes.data, i.ctypes.data, c.ctypes.data), None,
                 "czc_test_topk")
    return p, i, c


def bridge(tables: BridgeArrays, rows):
    lib = native.load_test()
    rows = np.ascontiguousarray(rows, np.int32)
    n, T = rows.shape
    ids = np.empty((n, native.CLIP_MAX_LEN), np.int32)
    ln = np.empty((n,), np.int32)
    st = tables.as_struct()
    native.check(lib.czc_test_bridge(C.byref(st), None, n, T, rows.ctypes.data, ids.ctypes.data, ln.ctypes.data), None,
                 "czc_test_bridge")
    return ids, ln


def combine(text_feat, img_embeds, logit_scale, probs, hyper, senti_raw=None, repeats=None):
    lib = native.load_test()
    tf = np.ascontiguousarray(text_feat, np.float32)
    ie = np.ascontiguousarray(img_embeds, np.float32)
    pr = np.ascontiguousarray(probs, np.float32)
    B, K = pr.shape
    D = ie.shape[1]
    sr = None if senti_raw is None else np.ascontiguousarray(senti_raw, np.float32)
    rp = None if repeats is None else np.ascontiguousarray(repeats, np.float32)
    cs, cr, fs = (np.empty((B, K), np.float32) for _ in range(3))
    best = np.empty((B,), np.int32)
    native.check(lib.czc_test_combine(B, K, D, tf.ctypes.data, ie.ctypes.data, C.c_float(logit_scale), pr.ctypes.data,
                                      _ptr(sr), _ptr(rp), C.byref(hyper), cs.ctypes.data, cr.ctypes.data,
                                      fs.ctypes.data, best.ctypes.data), None, "czc_test_combine")
    return cs, cr, fs, best


# ---- the integer and selection side of the screen-then-refine engine (czc_test_scan .. czc_test_combine_refine) ----------------------
GUARD = 64                  # include/conzic_hip_test.h CZC_TEST_GUARD: words in front of and behind every output of these hooks
SENTINEL = 0x5A5A5A5A       # what a word no kernel wrote reads back as (compare through .view(np.uint32))


class Guarded(dict):
    """name -> the n words of an output; .guards: name -> its 2 * GUARD guard words"""

    def __init__(self):
        super().__init__()
        self.guards = {}
        self._full = {}

    def buf(self, name, n, dtype=np.int32):
        self._full[name] = np.zeros(int(n) + 2 * GUARD, dtype)
        return self._full[name].ctypes.data

    def done(self):
        for name, full in self._full.items():
            self[name] = full[GUARD:full.size - GUARD]
            self.guards[name] = np.concatenate([full[:GUARD], full[full.size - GUARD:]])
        return self

    def assert_guards(self):
        for name, g in self.guards.items():
            bad = np.nonzero(g.view(np.uint32) != SENTINEL)[0]
            assert bad.size == 0, f"{name}: stray store into guard words {bad[:8].tolist()} (front: < {GUARD})"


def untouched(a):
    """mask of the words that still hold the pre-fill pattern"""
    return np.asarray(a).view(np.uint32) == SENTINEL


def scan(length):
    lib = native.load_test()
    ln = np.ascontiguousarray(length, np.int32)
    g = Guarded()
    native.check(lib.czc_test_scan(ln.size, ln.ctypes.data, g.buf("off", ln.size + 1), g.buf("totals", 2)), None, "czc_test_scan")
    return g.done()


def prefix_plan(ids, length, share, dedup):
    lib = native.load_test()
    ids = np.ascontiguousarray(ids, np.int32)
    ln = np.ascontiguousarray(length, np.int32)
    B, K = ln.shape
    assert ids.shape == (B, K, native.CLIP_MAX_LEN)
    S = B + B * K
    g = Guarded()
    native.check(lib.czc_test_prefix_plan(B, K, int(share), int(dedup), ids.ctypes.data, ln.ctypes.data, g.buf("own_len", S),
                                          g.buf("pre_len", S), g.buf("seg_src", S), g.buf("seg_pos0", S), g.buf("own_off", S + 1),
                                          g.buf("pre_off", S), g.buf("eos_idx", B * K), g.buf("rep", B * K), g.buf("img_max", B),
                                          g.buf("totals", 8)), None, "czc_test_prefix_plan")
    return g.done()


def refine_select(form, clip_score, final_score, m_samples, gate_h, need_cos, theta=0.0, beta=0.0, theta_base=0.0, scale=0.0,
                  hyper=None, draws=None):
    """form 0 scalar (theta, beta), 1 per-row hyper-parameters (theta_base, scale, hyper: list of native.Hyper), 2 drawing rows
    (draws: list of native.Draw; hyper or the scalars) -> Guarded(gated [2], kind, list [B, K], count [B])"""
    lib = native.load_test()
    cs = np.ascontiguousarray(clip_score, np.float32)
    fs = np.ascontiguousarray(final_score, np.float32)
    B, K = cs.shape
    hp = (native.Hyper * B)(*hyper) if hyper is not None else None
    dr = (native.Draw * B)(*draws) if draws is not None else None
    g = Guarded()
    native.check(lib.czc_test_refine_select(int(form), B, K, cs.ctypes.data, fs.ctypes.data, float(theta), float(theta_base), float(scale),
                                            int(m_samples), float(gate_h), float(beta), int(need_cos),
                                            C.cast(hp, C.c_void_p) if hp is not None else None,
                                            C.cast(dr, C.c_void_p) if dr is not None else None,
                                            g.buf("gated", 2), g.buf("kind", B * K), g.buf("list", B * K), g.buf("count", B)),
                 None, "czc_test_refine_select")
    g.done()
    g["kind"] = g["kind"].reshape(B, K)
    g["list"] = g["list"].reshape(B, K)
    return g


def refine_plan(clip_len, trunk_len, lst, count):
    lib = native.load_test()
    cl = np.ascontiguousarray(clip_len, np.int32)
    tl = np.ascontiguousarray(trunk_len, np.int32)
    ls = np.ascontiguousarray(lst, np.int32)
    ct = np.ascontiguousarray(count, np.int32)
    B, K = cl.shape
    S = B + B * K
    g = Guarded()
    native.check(lib.czc_test_refine_plan(B, K, cl.ctypes.data, tl.ctypes.data, ls.ctypes.data, ct.ctypes.data, g.buf("count_off", B + 1),
                                          g.buf("own_len", S), g.buf("pre_len", S), g.buf("seg_src", S), g.buf("seg_pos0", S),
                                          g.buf("own_off", S + 1), g.buf("pre_off", S), g.buf("rlist", B * K), g.buf("eos_idx", B * K),
                                          g.buf("img_max", B), g.buf("totals", 16)), None, "czc_test_refine_plan")
    return g.done()


def refine_cosine(feat, img, rlist, n_rows, B, K):
    lib = native.load_test()
    tf = np.ascontiguousarray(feat, np.float32)
    ie = np.ascontiguousarray(img, np.float32)
    rl = np.ascontiguousarray(rlist, np.int32)
    n_max, D = tf.shape
    assert rl.shape == (n_max,) and ie.shape == (B, D)
    g = Guarded()
    native.check(lib.czc_test_refine_cosine(n_max, int(n_rows), B, K, D, tf.ctypes.data, ie.ctypes.data, rl.ctypes.data,
                                            g.buf("cos_out", B * K, np.float32), g.buf("nonfinite", 8)), None, "czc_test_refine_cosine")
    return g.done()


def combine_refine(cos_in, probs, logit_scale, hyper, kind, rcos, guard):
    lib = native.load_test()
    ci = np.ascontiguousarray(cos_in, np.float32)
    pr = np.ascontiguousarray(probs, np.float32)
    kd = np.ascontiguousarray(kind, np.int32)
    rc = np.ascontiguousarray(rcos, np.float32)
    B, K = ci.shape
    g = Guarded()
    native.check(lib.czc_test_combine_refine(B, K, float(logit_scale), ci.ctypes.data, pr.ctypes.data, C.byref(hyper), kd.ctypes.data,
                                             rc.ctypes.data, float(guard), g.buf("clip_score", B * K, np.float32),
                                             g.buf("clip_ref", B * K, np.float32), g.buf("final_score", B * K, np.float32),
                                             g.buf("best", B), g.buf("best_cos", B, np.float32), g.buf("nonfinite", 8)),
                 None, "czc_test_combine_refine")
    return g.done()


# ---- the row, embedding, mover and memo kernels one by one (czc_test_layernorm_rows .. czc_test_memo_rows_chain) --------------------
# Outputs come back raw (include/conzic_hip_test.h): Stored decodes the bytes of an activation-typed buffer.
REFUSED = PLAN_REFUSED


def act_words(prec, n):
    return (int(n) * (2 if prec in (0, 4) else 4) + 3) // 4


class Stored:
    """n elements of precision `prec` as the kernel stored them: .bits (bf16 / fp16: uint16 patterns; f32: uint32; split: (hi, lo)
    uint16 patterns) and .f32 (their exact value in float32; split: float32(hi) + float32(lo), the kernels' own read)."""

    def __init__(self, prec, words, n):
        w = np.ascontiguousarray(words)
        if prec == 1:
            self.bits = w.view(np.uint32)[:n].copy()
            self.f32 = self.bits.view(np.float32)
        elif prec == 0:
            self.bits = w.view(np.uint16)[:n].copy()
            self.f32 = (self.bits.astype(np.uint32) << 16).view(np.float32)
        elif prec == 4:
            self.bits = w.view(np.uint16)[:n].copy()
            self.f32 = self.bits.view(np.float16).astype(np.float32)
        else:
            assert n % 8 == 0, "split rows are whole groups of 8 elements"
            g = w.view(np.uint16)[:2 * n].reshape(-1, 16)
            hi, lo = g[:, :8].reshape(-1).copy(), g[:, 8:].reshape(-1).copy()
            self.bits = (hi, lo)
            self.f32 = hi.view(np.float16).astype(np.float32) + lo.view(np.float16).astype(np.float32)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def _call(name, *args):
    """-> refused (the launcher returned its refusal status and launched nothing); any other non-zero status raises"""
    rc = getattr(native.load_test(), name)(*args)
    if rc != REFUSED:
        native.check(rc, None, name)
    return rc == REFUSED


def layernorm_rows(prec, x, gamma, beta, eps, row_idx=None, M=None, mode=3):
    """-> (refused, Guarded(y_act raw words, y_f32 [M*H])); mode 1 typed, 2 fp32, 4 in place (y_f32 = the x buffer)"""
    x = _f32(x)
    n_src, H = x.shape
    ri = _i32(row_idx)
    M = (ri.size if ri is not None else n_src) if M is None else M
    g = Guarded()
    ref = _call("czc_test_layernorm_rows", prec, M, H, n_src, x.ctypes.data, _ptr(ri), _f32(gamma).ctypes.data, _f32(beta).ctypes.data,
                float(eps), int(mode), g.buf("y_act", act_words(prec, M * H)), g.buf("y_f32", M * H, np.float32))
    return ref, g.done()


def layernorm_x16_rows(prec, x, gamma, beta, eps, row_idx=None):
    x = _f32(x)
    n_src, H = x.shape
    ri = _i32(row_idx)
    M = ri.size if ri is not None else n_src
    g = Guarded()
    ref = _call("czc_test_layernorm_x16_rows", prec, M, H, n_src, x.ctypes.data, _ptr(ri), _f32(gamma).ctypes.data, _f32(beta).ctypes.data,
                float(eps), g.buf("y_act", M * H // 2))
    return ref, g.done()


def layernorm_splitk(prec, slabs, H, bias, resid, gamma, beta, eps):
    """slabs [nslab, M, ld]; resid [M, ldr] or None"""
    s = _f32(slabs)
    nslab, M, ld = s.shape
    b = None if bias is None else _f32(bias)
    r = None if resid is None else _f32(resid)
    g = Guarded()
    ref = _call("czc_test_layernorm_splitk", prec, nslab, M, H, ld, s.ctypes.data, _ptr(b), _ptr(r), 0 if r is None else r.shape[1],
                _f32(gamma).ctypes.data, _f32(beta).ctypes.data, float(eps), g.buf("y_act", act_words(prec, M * H)),
                g.buf("y_f32", M * H, np.float32))
    return ref, g.done()


def ln_finalize(part, M, eps):
    """part [nblk, ld, 2] -> Guarded(stat [2*M])"""
    p = _f32(part)
    nblk, ld, _ = p.shape
    g = Guarded()
    ref = _call("czc_test_ln_finalize", nblk, M, ld, p.ctypes.data, float(eps), g.buf("stat", 2 * M, np.float32))
    return ref, g.done()


def bert_embed(prec, ids, word, pos, type0, gamma, beta, eps):
    ids = _i32(ids)
    B, T = ids.shape
    word, pos = _f32(word), _f32(pos)
    V, H = word.shape
    g = Guarded()
    ref = _call("czc_test_bert_embed", prec, B, T, H, V, pos.shape[0], ids.ctypes.data, word.ctypes.data, pos.ctypes.data,
                _f32(type0).ctypes.data, _f32(gamma).ctypes.data, _f32(beta).ctypes.data, float(eps),
                g.buf("y_act", act_words(prec, B * T * H)), g.buf("y_f32", B * T * H, np.float32))
    return ref, g.done()


def bert_embed_ragged(prec, ids, run, row_off, row_len, max_T, n_out_rows, word, pos, type0, gamma, beta, eps):
    ids = _i32(ids)
    n_id_rows, stride = ids.shape
    rn, ro, rl = _i32(run), _i32(row_off), _i32(row_len)
    word, pos = _f32(word), _f32(pos)
    V, H = word.shape
    g = Guarded()
    ref = _call("czc_test_bert_embed_ragged", prec, rl.size, n_id_rows, stride, int(max_T), H, V, pos.shape[0], ids.ctypes.data, _ptr(rn),
                ro.ctypes.data, rl.ctypes.data, int(n_out_rows), word.ctypes.data, pos.ctypes.data, _f32(type0).ctypes.data,
                _f32(gamma).ctypes.data, _f32(beta).ctypes.data, float(eps), g.buf("y_act", act_words(prec, n_out_rows * H)),
                g.buf("y_f32", n_out_rows * H, np.float32))
    return ref, g.done()


def clip_embed(mode, ids, seg_src, seg_pos0, own_off, own_len, max_len, n_out_rows, tok, pos, eps=0.0):
    ids = _i32(ids)
    n_id_rows, stride = ids.shape
    ss, sp, oo, ol = _i32(seg_src), _i32(seg_pos0), _i32(own_off), _i32(own_len)
    tok, pos = _f32(tok), _f32(pos)
    V, H = tok.shape
    g = Guarded()
    ref = _call("czc_test_clip_embed", int(mode), ol.size, int(max_len), H, n_id_rows, stride, ids.ctypes.data, ss.ctypes.data, sp.ctypes.data,
                oo.ctypes.data, ol.ctypes.data, V, pos.shape[0], tok.ctypes.data, pos.ctypes.data, int(n_out_rows), float(eps),
                g.buf("x", act_words(4 if mode else 1, n_out_rows * H)), g.buf("stat", 2 * n_out_rows, np.float32))
    return ref, g.done()


def im2col(prec, pix, p):
    pix = _f32(pix)
    B, _, S, _ = pix.shape
    n = B * (S // p) ** 2 * 3 * p * p
    g = Guarded()
    ref = _call("czc_test_im2col", prec, B, S, int(p), pix.ctypes.data, g.buf("out", act_words(prec, n)))
    return ref, g.done()


def vision_assemble(patch_out, cls, pos):
    po, pos = _f32(patch_out), _f32(pos)
    B, P, H = po.shape
    g = Guarded()
    ref = _call("czc_test_vision_assemble", B, P, H, po.ctypes.data, _f32(cls).ctypes.data, pos.ctypes.data, g.buf("x", B * (P + 1) * H, np.float32))
    return ref, g.done()


def l2_normalize(x):
    x = _f32(x)
    M, D = x.shape
    g = Guarded()
    ref = _call("czc_test_l2_normalize", M, D, x.ctypes.data, g.buf("y", M * D, np.float32))
    return ref, g.done()


def gather_rows(kind, src, idx, W):
    """kind 0 f32 rows of W floats, 1 rows of W bytes, 2 rows of W words; src [n_src, words per row] uint32"""
    s = np.ascontiguousarray(src, np.uint32)
    ix = _i32(idx)
    rw = W // 4 if kind == 1 else W
    assert s.shape[1] == rw
    g = Guarded()
    ref = _call("czc_test_gather_rows", int(kind), ix.size, int(W), s.shape[0], s.ctypes.data, ix.ctypes.data, g.buf("dst", ix.size * rw))
    return ref, g.done()


def mask_positions(inp, gen, n_mask, mask_id):
    """gen: an int (launch_mask_positions) or an array [B] (launch_mask_positions_rows)"""
    inp = _i32(inp)
    B, T = inp.shape
    rows = None if np.isscalar(gen) else _i32(gen)
    g = Guarded()
    ref = _call("czc_test_mask_positions", B, T, int(gen) if rows is None else 0, _ptr(rows), int(n_mask), int(mask_id), inp.ctypes.data,
                g.buf("inp", B * T))
    return ref, g.done()


def tie_rows(inp, col, grp_of_row, grp_off, grp_rows):
    inp = _i32(inp)
    R, T = inp.shape
    c, gr, go, rows = _i32(col), _i32(grp_of_row), _i32(grp_off), _i32(grp_rows)
    g = Guarded()
    ref = _call("czc_test_tie_rows", R, T, go.size - 1, inp.ctypes.data, c.ctypes.data, gr.ctypes.data, go.ctypes.data, rows.ctypes.data,
                g.buf("inp", R * T))
    return ref, g.done()


def memo_chain(st, gen_idx, n_mask, mask_id, n_sub, stages=1, use_list=1, record=1):
    """st: the arrays of tests/memo_ref.py MemoState (inp, key, img_max, img_n, new_rows, new_cos, new_max, ent_rows, ent_cos, ent_max,
    bcos) -> Guarded of every buffer the chain may write"""
    B, T = st["inp"].shape
    D = st["img_n"].shape[1]
    i = {k: _i32(st[k]) for k in ("inp", "key", "img_max", "new_rows", "new_max", "ent_rows", "ent_max")}
    f = {k: _f32(st[k]) for k in ("img_n", "new_cos", "ent_cos", "bcos")}
    g = Guarded()
    ref = _call("czc_test_memo_chain", B, T, D, int(gen_idx), int(n_mask), int(mask_id), int(n_sub), int(stages), int(use_list), int(record),
                i["inp"].ctypes.data, i["key"].ctypes.data, i["img_max"].ctypes.data, f["img_n"].ctypes.data, i["new_rows"].ctypes.data,
                f["new_cos"].ctypes.data, i["new_max"].ctypes.data, i["ent_rows"].ctypes.data, f["ent_cos"].ctypes.data,
                i["ent_max"].ctypes.data, f["bcos"].ctypes.data,
                g.buf("hit", B), g.buf("list", B), g.buf("tot", 4), g.buf("key", B * T), g.buf("inp", B * T), g.buf("bcos", B, np.float32),
                g.buf("ent_rows", B * T), g.buf("ent_cos", B, np.float32), g.buf("ent_max", B), g.buf("inp_c", B * T),
                g.buf("img_c", B * D, np.float32))
    return ref, g.done()


def memo_rows_chain(st, L, seed_len, n_mask0, n_sub, mask_id, j=0, stages=1, use_list=1, record=1):
    """st: the arrays of tests/memo_ref.py (inp, col0, col1 | None, tau | None, col, dot, img_n, new_rows, new_cos, new_max, bcos and the
    table valid, sig, key, rows, cos, imax)"""
    R, T = st["inp"].shape
    D = st["img_n"].shape[1]
    i = {k: _i32(st[k]) for k in ("inp", "col0", "col1", "col", "dot", "new_rows", "new_max", "valid", "sig", "key", "rows", "imax")}
    f = {k: (None if st[k] is None else _f32(st[k])) for k in ("tau", "img_n", "new_cos", "bcos", "cos")}
    nb = (R + 255) // 256
    g = Guarded()
    ref = _call("czc_test_memo_rows_chain", R, T, int(L), int(seed_len), D, int(n_mask0), int(n_sub), int(mask_id), int(j), int(stages),
                int(use_list), int(record), i["inp"].ctypes.data, i["col0"].ctypes.data, _ptr(i["col1"]), _ptr(f["tau"]), i["col"].ctypes.data,
                i["dot"].ctypes.data, f["img_n"].ctypes.data, i["new_rows"].ctypes.data, f["new_cos"].ctypes.data, i["new_max"].ctypes.data,
                f["bcos"].ctypes.data, i["valid"].ctypes.data, i["sig"].ctypes.data, i["key"].ctypes.data, i["rows"].ctypes.data,
                f["cos"].ctypes.data, i["imax"].ctypes.data,
                g.buf("valid", L * R), g.buf("sig", L * R), g.buf("key", L * R * T), g.buf("rows", L * 2 * R * T),
                g.buf("cos", L * 2 * R, np.float32), g.buf("imax", L * 2 * R), g.buf("hit", R), g.buf("cnt", nb), g.buf("list", R),
                g.buf("tot", 4), g.buf("inp", R * T), g.buf("bcos", R, np.float32), g.buf("inp_c", R * T), g.buf("img_c", R * D, np.float32),
                g.buf("col_c", R), g.buf("dot_c", R))
    return ref, g.done()


# ---- the text bridge with candidates and the per-row forms of the top-K selection (czc_test_bridge_cand, czc_test_topk_rows) ---------
# Compared with the string reference tests/bridge_ref.py (pinned by tests/test_bridge_ref_cpu.py) in tests/test_bridge_kernel_gpu.py,
# and with an fp64 softmax in tests/test_topk_rows_gpu.py.
def bridge_cand(tables: BridgeArrays, form, inp, gen, cand, row_len=None, lexicon=None, lex_pos=None, lex_cls=None, tag_of_token=None,
                masks=None, negative=0, hyper=None, K=None):
    """form 0 launch_bridge (gen: an int), 1 launch_bridge_rows, 2 launch_bridge_rows_hp (gen: [B] or None; hyper: list of native.Hyper
    or None).  cand [B, K] or None (then K names the launch's K).  -> (refused, Guarded(clip_ids [B*K, 77], clip_len, senti_raw,
    repeats [B*K], overflow [1]))"""
    inp = _i32(inp)
    B, T = inp.shape
    cd = _i32(cand)
    K = cd.shape[1] if cd is not None else int(K)
    assert cd is None or cd.shape == (B, K)
    rows = None if (form == 0 or gen is None) else _i32(gen)
    rl = _i32(row_len)
    lx = None if lexicon is None else _f32(lexicon)
    lp = None if lex_pos is None else _f32(lex_pos)
    lc = None if lex_cls is None else np.ascontiguousarray(lex_cls, np.uint8)
    tg = None if tag_of_token is None else np.ascontiguousarray(tag_of_token, np.uint8)
    mk = None if masks is None else np.ascontiguousarray(masks, np.uint16)
    hp = (native.Hyper * B)(*hyper) if hyper is not None else None
    st = tables.as_struct()
    g = Guarded()
    ref = _call("czc_test_bridge_cand", C.byref(st), int(form), B, T, K, inp.ctypes.data, int(gen) if form == 0 else 0, _ptr(rows), _ptr(rl),
                _ptr(cd), _ptr(lx), _ptr(lp), _ptr(lc), _ptr(tg), _ptr(mk), 0 if mk is None else mk.size, int(negative),
                C.cast(hp, C.c_void_p) if hp is not None else None,
                g.buf("clip_ids", B * K * native.CLIP_MAX_LEN), g.buf("clip_len", B * K), g.buf("senti_raw", B * K, np.float32),
                g.buf("repeats", B * K, np.float32), g.buf("overflow", 1))
    g.done()
    g["clip_ids"] = g["clip_ids"].reshape(B * K, native.CLIP_MAX_LEN)
    return ref, g


def topk_rows(form, logits, mask, K, dot_id, dot_rows, temperature=1.0, hyper=None):
    """form 1 launch_softmax_mask_topk_rows (temperature, dot_rows [B]), 2 launch_softmax_mask_topk_rows_hp (hyper: list of
    native.Hyper, dot_rows) -> (refused, Guarded(probs, idxs, cand [B, K]))"""
    lg = _f32(logits)
    mk = np.ascontiguousarray(np.asarray(mask, np.float32).reshape(-1))
    B, V = lg.shape
    dr = _i32(dot_rows)
    hp = (native.Hyper * B)(*hyper) if hyper is not None else None
    g = Guarded()
    ref = _call("czc_test_topk_rows", int(form), B, V, int(K), lg.ctypes.data, mk.ctypes.data, float(temperature), int(dot_id), _ptr(dr),
                C.cast(hp, C.c_void_p) if hp is not None else None, g.buf("probs", B * K, np.float32), g.buf("idxs", B * K),
                g.buf("cand", B * K))
    g.done()
    for k in ("probs", "idxs", "cand"):
        g[k] = g[k].reshape(B, K)
    return ref, g


# ---- every GEMM family on strided, windowed and in-place buffers (czc_test_gemm_layout; host side in tests/gemm_layout.py) ---------

def gemm_layout(case, data, eps=1e-5):
    """One GEMM launch of a gemm_layout.Case on the dense fp32 inputs `data` (gemm_layout.make_data) -> (launch, family):
    launch = gemm_layout.Launch, the Guarded of these hooks in two dimensions (name -> the WHOLE raw output buffer with its guard
    rows and pad columns, .part / .part_guards for the x16 form's row_part); family = the CZC_GEMM_FAMILY_* the launcher reported,
    0 when it refused the launch (nothing ran: every output is the untouched pattern)."""
    import gemm_layout as GL
    lib = native.load_test()
    c = case.filled()
    launch = GL.Launch(c)
    keep = {}

    def arr(name, need=True):
        if not need:
            return None
        keep[name] = np.ascontiguousarray(data[name], np.float32)
        return keep[name].ctypes.data

    for name, kind in c.outputs().items():
        launch[name] = np.zeros((launch.total_rows(), c.ldc * GL.ELEM_BYTES[kind]), np.uint8)
    part = np.zeros(2 * GUARD + c.N // 32 * c.part_ld * 2, np.float32) if c.part_ld else None
    s = native.GemmLayout(precision=c.prec, form=c.form, M=c.M, N=c.N, K=c.K, act=c.act, lda=c.lda, ldw=c.ldw, ldc=c.ldc, ldr=c.ldr,
                          c0=c.c0, flags=c.flags, part_ld=c.part_ld, eps=float(eps), A=arr("A"), W=arr("W"), bias=arr("bias", c.bias),
                          resid=arr("resid", c.has_resid), gamma=arr("gamma", c.form in (GL.LNF, GL.ROWLN)),
                          beta=arr("beta", c.form in (GL.LNF, GL.ROWLN)), ln_part=arr("ln_part", c.form == GL.LNF),
                          out_f32=launch["out_f32"].ctypes.data if "out_f32" in launch else None,
                          out_act=launch["out_act"].ctypes.data if "out_act" in launch else None, part_out=_ptr(part))
    rc = lib.czc_test_gemm_layout(C.byref(s))
    if rc < 0:
        native.check(-rc, None, "czc_test_gemm_layout")
    launch.family = rc
    if part is not None:
        launch.part = part[GUARD:part.size - GUARD].reshape(c.N // 32, c.part_ld, 2)
        launch.part_guards = np.concatenate([part[:GUARD], part[part.size - GUARD:]])
    return launch, rc


# czc_test_set_option defaults of the GEMM launchers (csrc/gemm.hip, gemm256.hip, gemm_wreg.hip)
GEMM_OPTION_DEFAULTS = {"gemm256": 1, "skinny": 1, "splitk": 1, "gemm_deep": 1, "gemm_small_tiles": 4, "wreg": 1, "gemm256s": 1, "rowln_min_m": 8192,
                        "wreg_min_m": 1, "gemm256_min_m": 8192, "gemm256s_min_m": 16384, "wreg_resid_min_m": 6144, "wreg_stats_in_kernel": 1}


@contextlib.contextmanager
def gemm_options(**kw):
    """pins kernel switches and thresholds for the launches inside, and puts the defaults back whatever happens"""
    lib = native.load_test()
    try:
        for k, v in kw.items():
            assert lib.czc_test_set_option(k.encode(), int(v)) == 0, k
        yield
    finally:
        for k in kw:
            lib.czc_test_set_option(k.encode(), GEMM_OPTION_DEFAULTS[k])
