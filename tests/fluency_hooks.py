"""ctypes wrappers of the caption-fluency hooks of libconzic_hip_test.so (include/conzic_hip_test.h).  TEST INFRASTRUCTURE."""
import numpy as np

from conzic_amd import native
from conzic_amd.engine import _ptr


def logprob(logits, target, temperature):
    """launch_logprob_target on logits [N, V] / target [N] -> (logp fp32 [N], rank int32 [N], nonfinite flag)."""
    lib = native.load_test()
    x = np.ascontiguousarray(logits, dtype=np.float32)
    t = np.ascontiguousarray(target, dtype=np.int32)
    N, V = x.shape
    assert t.shape == (N,)
    logp, rank = np.empty((N,), np.float32), np.empty((N,), np.int32)
    flag = np.zeros((1,), np.int32)
    native.check(lib.czc_test_logprob(N, V, x.ctypes.data, t.ctypes.data, float(temperature), logp.ctypes.data, rank.ctypes.data,
                                      flag.ctypes.data), None, "czc_test_logprob")
    return logp, rank, int(flag[0])


def expand_mask(rows, seed_len, mask_id, lens=None):
    """The expansion of czc_fluency_rows on rows [R, T] -> (ids [N, T], target [N], gen_rows [N])."""
    lib = native.load_test()
    r = np.ascontiguousarray(rows, dtype=np.int32)
    R, T = r.shape
    ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    n_max = R * max(T - seed_len - 1, 1)
    ids, target, gen = np.empty((n_max, T), np.int32), np.empty((n_max,), np.int32), np.empty((n_max,), np.int32)
    n = np.zeros((1,), np.int32)
    native.check(lib.czc_test_expand_mask(R, T, int(seed_len), int(mask_id), r.ctypes.data, _ptr(ln), ids.ctypes.data, target.ctypes.data,
                                          gen.ctypes.data, n.ctypes.data), None, "czc_test_expand_mask")
    N = int(n[0])
    return ids[:N].copy(), target[:N].copy(), gen[:N].copy()
