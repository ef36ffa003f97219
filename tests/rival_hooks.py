"""The kernel-level hook of the rival combine (czc_test_combine_rivals, include/conzic_hip_test.h) as a typed numpy wrapper.
TEST INFRASTRUCTURE, like tests/kernel_hooks.py: nothing in conzic_amd/ imports this module."""
import ctypes as C

import numpy as np

from conzic_amd import native
from conzic_amd.engine import draw_array, hyper_array
from kernel_hooks import Guarded


def combine_rivals(text_feat, img_all, image_of_row, rival_idx, delta, logit_scale, probs, hypers, draws=None, step=0):
    """B rows with own image image_of_row[b] of img_all [n_img, D] and rivals rival_idx [B, M] into img_all ->
    Guarded(clip_ref, disc, final_score [B, K]; best [B]; nonfinite [8])."""
    lib = native.load_test()
    tf = np.ascontiguousarray(text_feat, np.float32)
    ia = np.ascontiguousarray(img_all, np.float32)
    pr = np.ascontiguousarray(probs, np.float32)
    ior = np.ascontiguousarray(image_of_row, np.int32).reshape(-1)
    rv = np.ascontiguousarray(rival_idx, np.int32)
    dl = np.ascontiguousarray(delta, np.float32).reshape(-1)
    B, K = pr.shape
    n_img, D = ia.shape
    assert tf.shape == (B * K, D) and ior.size == B and rv.shape[0] == B and dl.size == B
    hp = hyper_array(hypers)
    dr = None if draws is None else draw_array(draws)
    assert len(hp) == B and (dr is None or len(dr) == B)
    g = Guarded()
    native.check(lib.czc_test_combine_rivals(B, K, D, tf.ctypes.data, ia.ctypes.data, n_img, ior.ctypes.data, rv.ctypes.data,
                                             int(rv.shape[1]), dl.ctypes.data, C.c_float(logit_scale), pr.ctypes.data, hp, dr,
                                             int(step), g.buf("clip_ref", B * K, np.float32), g.buf("disc", B * K, np.float32),
                                             g.buf("final_score", B * K, np.float32), g.buf("best", B), g.buf("nonfinite", 8)),
                 None, "czc_test_combine_rivals")
    g.done()
    for name in ("clip_ref", "disc", "final_score"):
        g[name] = g[name].reshape(B, K)
    return g
