"""NumPy float64 reference of the rival combine (conzic_amd/csrc/combine.hip: cosine_rival_kernel and the RIVAL instantiation of
combine_kernel), for tests/test_rival_kernel_gpu.py.  The formula itself is conzic_amd.rivals.disc_ref."""
import numpy as np

from conzic_amd import rivals

BAR_COS = 1e-6   # per unit of exp(logit_scale): the project's bar on an fp32 cosine against fp64 is 2e-6, two cosines enter each
                 # exponent x_j = s (cj - c0), and sum_j |d disc / d x_j| = disc (1 - disc) <= 1/4  ->  |d disc| <= s * 4e-6 / 4


def disc_bar(scale):
    return float(scale) * BAR_COS


def normalise(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def combine(text_feat, img_all, image_of_row, rival_idx, delta, logit_scale, probs, alpha, beta):
    """-> dict(cos [B, K], disc [B, K], final [B, K], final0 [B, K] (without the rival term)), all float64.  alpha, beta: scalars
    or [B]."""
    pr = np.asarray(probs, dtype=np.float64)
    B, K = pr.shape
    ia = normalise(img_all)
    t = normalise(np.asarray(text_feat, dtype=np.float64).reshape(B, K, -1))
    ior = np.asarray(image_of_row).reshape(-1)
    rv = np.asarray(rival_idx)
    s = float(np.exp(np.float64(logit_scale)))
    cos = np.einsum("bkd,bd->bk", t, ia[ior])
    cj = np.einsum("bkd,bmd->bkm", t, ia[np.maximum(rv, 0)])
    valid = np.broadcast_to((rv >= 0)[:, None, :], cj.shape)
    disc = rivals.disc_ref(cos, cj, s, valid)
    lg = cos * s
    cs = np.exp(lg - lg.max(axis=1, keepdims=True))
    cs /= cs.sum(axis=1, keepdims=True)
    al = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (B,))[:, None]
    be = np.broadcast_to(np.asarray(beta, dtype=np.float64), (B,))[:, None]
    final0 = al * pr + be * cs
    on = (np.asarray(delta, dtype=np.float64) != 0) & (rv[:, 0] >= 0)
    final = final0 + np.where(on, np.asarray(delta, dtype=np.float64), 0.0)[:, None] * disc
    return {"cos": cos, "disc": disc, "final": final, "final0": final0, "scale": s}


def top2_margin(final):
    """[B]: the gap between the best and the second-best score of every row (inf at K = 1)."""
    f = np.asarray(final, dtype=np.float64)
    if f.shape[1] < 2:
        return np.full(f.shape[0], np.inf)
    top = -np.partition(-f, 1, axis=1)[:, :2]
    return top[:, 0] - top[:, 1]
