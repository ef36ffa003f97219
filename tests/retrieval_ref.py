"""fp64 reference of the index search (czc_index_search): both sides L2-normalised, scores = q @ X.T, per query the rows
ordered by (cosine descending, id ascending)."""
import numpy as np


def normalize(a):
    a = np.asarray(a, dtype=np.float64)
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def scores(queries, index):
    """fp64 cosines [Q, N] of un-normalised queries [Q, D] against un-normalised index rows [N, D]."""
    return normalize(np.atleast_2d(queries)) @ normalize(np.atleast_2d(index)).T


def order(score_row):
    """Row ids of one score row under the total order (cosine descending, id ascending)."""
    s = np.asarray(score_row, dtype=np.float64)
    return np.lexsort((np.arange(s.size), -s))


def search(queries, index, k):
    """(ids int32 [Q, k], cosines fp64 [Q, k]); behind the index's last row the tail is (-1, -inf)."""
    sc = scores(queries, index)
    Q, N = sc.shape
    ids = np.full((Q, k), -1, dtype=np.int32)
    cos = np.full((Q, k), -np.inf, dtype=np.float64)
    for q in range(Q):
        o = order(sc[q])[:k]
        ids[q, :o.size] = o
        cos[q, :o.size] = sc[q, o]
    return ids, cos
