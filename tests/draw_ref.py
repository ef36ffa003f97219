"""NumPy reference of the seeded draw of czc_generate_rows_draw (include/conzic_hip.h), for tests/: Philox4x32-10 in uint64
arithmetic, everything behind it in float64, plus a ctypes wrapper of the kernel-level hook czc_test_combine_draw
(include/conzic_hip_test.h).

TEST INFRASTRUCTURE: written from the header's statement of the draw, not from the kernel."""
import ctypes as C

import numpy as np

from conzic_amd import native
from conzic_amd.engine import _ptr, draw_array

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xffffffff)
NEAR_TIE = 1e-4        # a draw whose best and second z lie within NEAR_TIE * (1 + |z_best|) may go either way in fp32
NEAR_TIE_CAP = 0.01    # ... and at most this share of the draws of one test may be such


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (broadcastable; any unsigned values < 2^32) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & MASK32
    k = np.asarray(key, dtype=np.uint64) & MASK32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0 = np.uint64(M0) * c0      # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def words(seed, step, K):
    """x_k for k in [0, K): seed int or uint64 [B], step int or [B] -> uint32 [B, K] (or [K] for scalar seed and step)."""
    seed = np.asarray(seed, dtype=np.uint64)
    step = np.asarray(step, dtype=np.uint64)
    scalar = seed.ndim == 0 and step.ndim == 0
    seed, step = np.broadcast_arrays(np.atleast_1d(seed), np.atleast_1d(step))
    nblk = (K + 3) // 4
    B = seed.shape[0]
    ctr = np.zeros((B, nblk, 4), dtype=np.uint64)
    ctr[..., 0] = step[:, None]
    ctr[..., 1] = np.arange(nblk, dtype=np.uint64)[None, :]
    key = np.stack([seed & MASK32, seed >> np.uint64(32)], axis=-1)[:, None, :]
    x = philox4x32_10(ctr, key).reshape(B, nblk * 4)[:, :K]
    return x[0] if scalar else x


def uniform(x):
    """u = ((x >> 9) + 0.5) * 2^-23, float64 (every value is an fp32 number)."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(x):
    return -np.log(-np.log(uniform(x)))


def perturbed(final, probs, seed, tau, step):
    """z [B, K] float64 for rows that all draw (tau > 0, scalar or [B])."""
    final = np.asarray(final, dtype=np.float64)
    B, K = final.shape
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (B,))[:, None]
    z = final / tau + gumbel(words(np.broadcast_to(np.asarray(seed, dtype=np.uint64), (B,)), step, K))
    return np.where(np.asarray(probs) == 0, -np.inf, z)


def winners(final, probs, seed, tau, step):
    """(winner int [B], near_tie bool [B]): the reference's draw per row.  tau [B] may hold zeros: such a row, and a row without
    an eligible candidate, takes the first argmax of `final`.  near_tie: the gap between the best and the second z is below
    NEAR_TIE * (1 + |z_best|) (never set for an argmax row)."""
    final = np.asarray(final, dtype=np.float64)
    B, K = final.shape
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (B,))
    draws = tau > 0
    z = perturbed(final, probs, seed, np.where(draws, tau, 1.0), step)
    win = np.argmax(final, axis=1)
    tie = np.zeros(B, dtype=bool)
    elig = draws & np.isfinite(z).any(axis=1)
    if elig.any():
        ze = z[elig]
        w = np.argmax(ze, axis=1)
        win[elig] = w
        if K > 1:
            top2 = -np.partition(-ze, 1, axis=1)[:, :2]
            gap = top2[:, 0] - top2[:, 1]
            tie[elig] = gap < NEAR_TIE * (1.0 + np.abs(top2[:, 0]))
    return win, tie


def make_draws(seeds, taus, step0=0):
    seeds = [int(s) for s in np.asarray(seeds, dtype=np.uint64).reshape(-1)]
    taus = np.broadcast_to(np.asarray(taus, dtype=np.float32), (len(seeds),))
    return [native.Draw(s, float(t), int(step0)) for s, t in zip(seeds, taus)]


def combine_draw(text_feat, img_embeds, logit_scale, probs, hyper, draws, step, senti_raw=None, repeats=None):
    """czc_test_combine_draw: the combine kernel's drawing instantiation on host data -> (final_score [B, K], best [B])."""
    lib = native.load_test()
    tf = np.ascontiguousarray(text_feat, np.float32)
    ie = np.ascontiguousarray(img_embeds, np.float32)
    pr = np.ascontiguousarray(probs, np.float32)
    B, K = pr.shape
    D = ie.shape[1]
    sr = None if senti_raw is None else np.ascontiguousarray(senti_raw, np.float32)
    rp = None if repeats is None else np.ascontiguousarray(repeats, np.float32)
    dr = draw_array(draws)
    assert len(dr) == B
    fs = np.empty((B, K), np.float32)
    best = np.empty((B,), np.int32)
    native.check(lib.czc_test_combine_draw(B, K, D, tf.ctypes.data, ie.ctypes.data, C.c_float(logit_scale), pr.ctypes.data,
                                           _ptr(sr), _ptr(rp), C.byref(hyper), dr, int(step), fs.ctypes.data, best.ctypes.data),
                 None, "czc_test_combine_draw")
    return fs, best


# ---- the inputs of tests/test_combine_draw_gpu.py (the CPU suite asserts the reference's near-tie share on these very arrays) ----
COMBINE_CASES = [(4096, 8), (64, 200), (4, 1024), (3, 1)]   # (B, K) at D = 64
COMBINE_D = 64
COMBINE_TAUS = (0.05, 0.5)
COMBINE_STEPS = (0, 7)
LOGIT_SCALE = 2.6592


def combine_inputs(B, K, senti=False, seed=0):
    """text_feat [B*K, D], image embeds [B, D], probs [B, K] (a softmax, so no zero), row seeds [B], and with `senti` the
    sentiment scores and repeat penalties."""
    rng = np.random.default_rng(1000 * K + B + seed)
    tf = rng.standard_normal((B * K, COMBINE_D)).astype(np.float32)
    ie = rng.standard_normal((B, COMBINE_D)).astype(np.float32)
    lg = rng.standard_normal((B, K)) * 2.0
    pr = np.exp(lg - lg.max(axis=1, keepdims=True))
    pr = (pr / pr.sum(axis=1, keepdims=True)).astype(np.float32)
    seeds = rng.integers(0, 2 ** 64, size=B, dtype=np.uint64)
    sr = rng.standard_normal((B, K)).astype(np.float32) if senti else None
    rp = (-rng.integers(0, 3, size=(B, K))).astype(np.float32) if senti else None
    return tf, ie, pr, seeds, sr, rp


def fused_ref(tf, ie, pr, alpha, beta, sr=None, rp=None, gamma=0.0):
    """float64 fused score of the combine kernel (clip/clip.py:91-98, gen_utils.py:77, control_gen_utils.py:59): what the CPU
    suite draws from where it has no device to ask for final_score."""
    B, K = pr.shape
    t = tf.astype(np.float64).reshape(B, K, -1)
    t = t / np.linalg.norm(t, axis=2, keepdims=True)
    i = ie.astype(np.float64)
    i = i / np.linalg.norm(i, axis=1, keepdims=True)
    lg = np.einsum("bkd,bd->bk", t, i) * np.exp(LOGIT_SCALE)
    cs = np.exp(lg - lg.max(axis=1, keepdims=True))
    cs /= cs.sum(axis=1, keepdims=True)
    f = alpha * pr.astype(np.float64) + beta * cs
    if sr is not None:
        sp = np.exp(sr - sr.max(axis=1, keepdims=True))
        f = f + gamma * sp / sp.sum(axis=1, keepdims=True) + 0.1 * (1.0 - np.exp(rp.astype(np.float64)))
    return f
