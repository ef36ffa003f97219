"""Rival images for czc_generate_rows_vs (include/conzic_hip.h): host-side tables, the counterpart of blocks.py and draws.py.

A row of a rivals call is scored against its own image i0 and up to M rivals i1..im of the resident batch.  For a candidate
sentence t the engine forms

    disc = softmax over {i0, i1..im} of exp(logit_scale) * cos(t, ij), taken at i0 = 1 / (1 + sum_j exp(s * (cj - c0)))

the probability that the caption retrieves its own image among the set, and adds delta * disc to the candidate's fused score.
This module builds the [B, M] table of an image batch (the nearest other images of each image's set), maps it to rows, and
states the formula in float64 (the reference the tests hold the kernel to).  No GPU, no engine.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

MAX_RIVALS = 16  # include/conzic_hip.h CZC_MAX_RIVALS


def rival_table(embeds, M: int, sets: Optional[Sequence[int]] = None,
                group_of_image: Optional[Sequence[int]] = None) -> np.ndarray:
    """int32 [B, M]: for image b the up to M OTHER images of its set with the highest image-image cosine (float64), best first,
    ties broken by the lowest index; -1 fills the tail of a set smaller than M + 1.  `sets` int [B]: the set id of every image
    (None: the whole batch is one set).  `embeds` [B, D] need not be normalised.
    `group_of_image` int [B]: the picture every image of the batch was cut from (conzic_amd.regions): an image's rivals are
    chosen among the images of its own group only, so the regions of one picture become each other's rivals and a group of one
    gets none.  With `sets` as well, a rival shares both.  None: the function is what it was."""
    if group_of_image is not None:
        grp = np.asarray(group_of_image, dtype=np.int64).reshape(-1)
        if sets is None:
            sets = grp
        else:
            st = np.asarray(sets, dtype=np.int64).reshape(-1)
            if st.size != grp.size:
                raise ValueError(f"rival_table: sets has {st.size} entries and group_of_image {grp.size}")
            _, sets = np.unique(np.stack([st, grp], axis=1), axis=0, return_inverse=True)   # one id per (set, group) pair
            sets = np.asarray(sets).reshape(-1)
    e = np.asarray(embeds, dtype=np.float64)
    if e.ndim != 2 or e.shape[0] < 1:
        raise ValueError(f"rival_table: embeds must be [B, D], got {e.shape}")
    if not 1 <= int(M) <= MAX_RIVALS:
        raise ValueError(f"rival_table: M = {M} outside [1, {MAX_RIVALS}]")
    B = e.shape[0]
    st = np.zeros((B,), np.int64) if sets is None else np.asarray(sets, dtype=np.int64).reshape(-1)
    if st.size != B:
        raise ValueError(f"rival_table: sets has {st.size} entries for {B} images")
    nrm = np.linalg.norm(e, axis=1, keepdims=True)
    if not np.all(np.isfinite(nrm)) or np.any(nrm == 0):
        raise ValueError("rival_table: an embedding with a zero or non-finite norm")
    en = e / nrm
    cos = en @ en.T
    out = np.full((B, int(M)), -1, dtype=np.int32)
    for b in range(B):
        others = [j for j in range(B) if j != b and st[j] == st[b]]
        others.sort(key=lambda j: (-cos[b, j], j))   # highest cosine first, the lowest index among equals
        out[b, :min(len(others), int(M))] = others[:int(M)]
    return out


def expand(table, image_of_row) -> np.ndarray:
    """int32 [R, M]: the table row of every row's own image."""
    t = np.asarray(table, dtype=np.int32)
    ior = np.asarray(image_of_row, dtype=np.int64).reshape(-1)
    if t.ndim != 2:
        raise ValueError(f"expand: table must be [B, M], got {t.shape}")
    if ior.size and (ior.min() < 0 or ior.max() >= t.shape[0]):
        raise ValueError("expand: image_of_row outside the table")
    return np.ascontiguousarray(t[ior])


def disc_ref(cos_own, cos_rivals, scale: float, valid=None) -> np.ndarray:
    """The formula in float64: cos_own [...], cos_rivals [..., m] (valid [..., m] bool, None: every slot counts), scale =
    exp(logit_scale) -> disc [...] = 1 / (1 + sum_j exp(scale * (cj - c0))), evaluated with max(0, max_j x_j) subtracted."""
    c0 = np.asarray(cos_own, dtype=np.float64)
    cj = np.asarray(cos_rivals, dtype=np.float64)
    x = float(scale) * (cj - c0[..., None])
    if valid is not None:
        x = np.where(np.asarray(valid, dtype=bool), x, -np.inf)
    mx = np.maximum(0.0, x.max(axis=-1)) if x.shape[-1] else np.zeros(c0.shape)
    with np.errstate(under="ignore"):
        den = np.exp(-mx) + np.exp(x - mx[..., None]).sum(axis=-1)
        return np.exp(-mx) / den


def check_table(table, image_of_row, n_images: int) -> None:
    """The refusals of the C call, as ValueError, for callers that build tables by hand."""
    t = np.asarray(table)
    ior = np.asarray(image_of_row).reshape(-1)
    if t.ndim != 2 or t.shape[0] != ior.size or not 1 <= t.shape[1] <= MAX_RIVALS:
        raise ValueError(f"rivals must be [R, M] with 1 <= M <= {MAX_RIVALS}, got {t.shape} for {ior.size} rows")
    if t.size and (t.min() < -1 or t.max() >= n_images):
        raise ValueError("a rival index outside [-1, resident image batch)")
    if np.any(t == ior[:, None]):
        raise ValueError("a rival equal to the row's own image")
    filled = t >= 0
    if np.any(filled[:, 1:] & ~filled[:, :-1]):
        raise ValueError("a filled rival slot behind an empty one")
