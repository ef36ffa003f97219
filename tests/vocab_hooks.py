"""Python side of czc_test_topk_rows_vocab (include/conzic_hip_test.h): the top-K selection with a vocabulary set per row, launched
alone.  The guard-word outputs and the refusal convention are those of tests/kernel_hooks.py."""
import ctypes as C

import numpy as np

import kernel_hooks as KH
from conzic_amd import native


def topk_rows_vocab(logits, mask, K, dot_id, dot_rows, hyper, set_rows, bits):
    """launch_softmax_mask_topk_rows_vocab: hyper (list of native.Hyper) and dot_rows [B] as in kernel_hooks.topk_rows form 2,
    set_rows int [B] in [-1, n_sets), bits uint32 [n_sets, W]; any of the four may be None (the launcher refuses)
    -> (refused, Guarded(probs, idxs, cand [B, K]))"""
    lg = KH._f32(logits)
    mk = np.ascontiguousarray(np.asarray(mask, np.float32).reshape(-1))
    B, V = lg.shape
    dr, sr = KH._i32(dot_rows), KH._i32(set_rows)
    bt = None if bits is None else np.ascontiguousarray(bits, np.uint32)
    assert bt is None or bt.ndim == 2
    hp = (native.Hyper * B)(*hyper) if hyper is not None else None
    g = KH.Guarded()
    ref = KH._call("czc_test_topk_rows_vocab", B, V, int(K), lg.ctypes.data, mk.ctypes.data, int(dot_id), KH._ptr(dr),
                   C.cast(hp, C.c_void_p) if hp is not None else None, KH._ptr(sr), KH._ptr(bt),
                   0 if bt is None else int(bt.shape[0]), (V + 31) // 32 if bt is None else int(bt.shape[1]),
                   g.buf("probs", B * K, np.float32), g.buf("idxs", B * K), g.buf("cand", B * K))
    g.done()
    for k in ("probs", "idxs", "cand"):
        g[k] = g[k].reshape(B, K)
    return ref, g
