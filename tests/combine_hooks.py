"""The kernel-level hook of the combine kernel's instantiations without rivals (czc_test_combine_rows, include/conzic_hip_test.h)
as a typed numpy wrapper.  TEST INFRASTRUCTURE, like tests/kernel_hooks.py: nothing in conzic_amd/ imports this module."""
import ctypes as C

import numpy as np

from conzic_amd import native
from conzic_amd.engine import _ptr, draw_array, hyper_array
from kernel_hooks import REFUSED, Guarded

FLOATS = ("clip_score", "clip_ref", "final_score")


def hyper(alpha, beta, gamma=0.0, control=0):
    return native.Hyper(float(alpha), float(beta), float(gamma), 1.0, int(control), 0)


def _f32(x):
    return None if x is None else np.ascontiguousarray(x, np.float32)


def combine_rows(logit_scale, probs, hypers, form=0, cos=None, text_feat=None, img=None, cand=None, senti_raw=None, repeats=None,
                 draws=None, step=0, gen_idx=0, gen_rows=None, inp=None, run=None):
    """One launch_combine on B rows (the shape of probs).  hypers: one native.Hyper (forms 0, 1) or a list (forms 2, 3; the full R
    records when `run` is given).  cos [B, K] or text_feat [B*K, D] + img [B, D].  inp [B, T] or None.
    -> (refused, Guarded(clip_score, clip_ref, final_score [B, K]; best, best_cos [B]; nonfinite [8]; inp [B, T] if given; hp
    [B, 6] / draw [B, 4] raw words if `run` is given))"""
    lib = native.load_test()
    pr = _f32(probs)
    B, K = pr.shape
    ci, tf, ie, sr, rp = _f32(cos), _f32(text_feat), _f32(img), _f32(senti_raw), _f32(repeats)
    D = 0 if ie is None else int(ie.shape[1])
    assert ci is None or ci.shape == (B, K)
    assert tf is None or tf.shape == (B * K, D)
    cd = np.zeros((B, K), np.int32) if cand is None else np.ascontiguousarray(cand, np.int32)
    hs = [hypers] if isinstance(hypers, native.Hyper) else list(hypers)
    hp = hyper_array(hs)
    dr = None if draws is None else draw_array(draws)
    rn = None if run is None else np.ascontiguousarray(run, np.int32).reshape(-1)
    R = len(hs)
    assert rn is None or rn.size == B
    assert form < 2 or rn is not None or R == B
    gr = None if gen_rows is None else np.ascontiguousarray(gen_rows, np.int32).reshape(-1)
    ip = None if inp is None else np.ascontiguousarray(inp, np.int32)
    T = 0 if ip is None else int(ip.shape[1])
    g = Guarded()
    scale = C.c_float(0.0)
    rc = lib.czc_test_combine_rows(B, K, D, T, _ptr(tf), _ptr(ie), _ptr(ci), C.c_float(logit_scale), pr.ctypes.data, cd.ctypes.data,
                                   _ptr(sr), _ptr(rp), int(form), hp, dr, int(step), int(gen_idx), _ptr(gr), _ptr(rn), R, _ptr(ip),
                                   g.buf("inp", B * T) if ip is not None else None,
                                   g.buf("clip_score", B * K, np.float32), g.buf("clip_ref", B * K, np.float32),
                                   g.buf("final_score", B * K, np.float32), g.buf("best", B), g.buf("best_cos", B, np.float32),
                                   g.buf("nonfinite", 8), g.buf("hp", B * 6) if rn is not None else None,
                                   g.buf("draw", B * 4) if rn is not None and form == 3 else None, C.addressof(scale))
    if rc != REFUSED:
        native.check(rc, None, "czc_test_combine_rows")
    g.done()
    g.scale = float(scale.value)   # expf(logit_scale) in fp32, as the kernel was handed it
    for name in FLOATS:
        g[name] = g[name].reshape(B, K)
    if ip is not None:
        g["inp"] = g["inp"].reshape(B, T)
    if rn is not None:
        g["hp"] = g["hp"].reshape(B, 6)
        if form == 3:
            g["draw"] = g["draw"].reshape(B, 4)
    return rc == REFUSED, g


def record_words(records):
    """the 4-byte words of a ctypes array of records, one row per record"""
    n = len(records)
    return np.frombuffer(bytes(records), np.int32).reshape(n, -1) if n else np.zeros((0, 0), np.int32)


def bits(a):
    return np.asarray(a).view(np.uint32)
