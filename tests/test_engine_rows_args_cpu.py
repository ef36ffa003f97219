"""The argument checks of Engine.generate_rows*: every array argument of every method, handed over with a wrong size or rank,
is refused with a ValueError that names the method and the argument -- before the library is touched (no GPU, no library)."""
import numpy as np
import pytest

from conzic_amd import native
from conzic_amd.engine import Engine

R, T, N_STEPS, L, SEED_LEN, TOP_K = 3, 9, 4, 4, 4, 8


def good_args():
    """every argument any of the seven methods takes, well-formed for R rows, T tokens and N_STEPS steps"""
    return dict(init_ids=np.zeros((T,), np.int32), init_rows=np.zeros((R, T), np.int32), L=L, lens=[2, 3, 4], seed_len=SEED_LEN,
                top_k=TOP_K, positions=np.zeros((N_STEPS, R), np.int32), hyper=Engine.hyper(0.02, 2.0, 0.1),
                hypers=[Engine.hyper(0.02, 2.0, 0.1) for _ in range(R)], draws=[native.Draw(r, 0.0, 0) for r in range(R)],
                groups=[0, 0, 2], rivals=np.full((R, 2), -1, np.int32), deltas=[0.0] * R, image_of_row=[0, 0, 1],
                n_mask=[1] * N_STEPS)


# method -> its parameters in order; the array ones with a wrong size or rank each
METHODS = {
    "generate_rows": ("init_ids", "L", "seed_len", "top_k", "positions", "hyper", "image_of_row", "n_mask"),
    "generate_rows_from": ("init_rows", "L", "seed_len", "top_k", "positions", "hyper", "image_of_row", "n_mask"),
    "generate_rows_len": ("init_rows", "lens", "seed_len", "top_k", "positions", "hyper", "image_of_row", "n_mask"),
    "generate_rows_hp": ("init_rows", "lens", "seed_len", "top_k", "positions", "hypers", "image_of_row", "n_mask"),
    "generate_rows_draw": ("init_rows", "lens", "seed_len", "top_k", "positions", "hypers", "draws", "image_of_row", "n_mask"),
    "generate_rows_tied": ("init_rows", "lens", "seed_len", "top_k", "positions", "hypers", "draws", "groups", "image_of_row"),
    "generate_rows_vs": ("init_rows", "lens", "seed_len", "top_k", "positions", "hypers", "draws", "groups", "rivals", "deltas",
                         "image_of_row", "n_mask"),
}
BAD = {
    "init_rows": [np.zeros((R - 1, T), np.int32), np.zeros((R * T,), np.int32), np.zeros((R, 0), np.int32)],
    "lens": [[2, 3], [[2, 3, 4], [2, 3, 4]]],
    "positions": [np.zeros((N_STEPS,), np.int32), np.zeros((N_STEPS, R, 1), np.int32), np.zeros((N_STEPS, 0), np.int32)],
    "hypers": [[Engine.hyper(0.02, 2.0, 0.1)] * (R - 1), [Engine.hyper(0.02, 2.0, 0.1)] * (R + 1)],
    "draws": [[native.Draw(0, 0.0, 0)] * (R - 1), []],
    "groups": [[0, 0], [0, 0, 1, 1]],
    "rivals": [np.full((R - 1, 2), -1, np.int32), np.full((R,), -1, np.int32), np.full((R, 0), -1, np.int32)],
    "deltas": [[0.0] * (R + 1), [0.0]],
    "image_of_row": [[0, 1], [0, 0, 1, 1]],
    "n_mask": [[1] * (N_STEPS - 1), [1] * (N_STEPS + 1)],
}
CASES = [(m, a, i) for m, params in METHODS.items() for a in params if a in BAD for i in range(len(BAD[a]))]


@pytest.mark.parametrize("method,arg,i", CASES, ids=[f"{m}-{a}-{i}" for m, a, i in CASES])
def test_a_wrong_size_or_rank_is_refused_by_name_before_the_library(method, arg, i):
    eng = Engine.__new__(Engine)   # no library, no handle: whatever touches either raises AttributeError, not ValueError
    kw = {k: v for k, v in good_args().items() if k in METHODS[method]}
    kw[arg] = BAD[arg][i]
    with pytest.raises(ValueError) as ei:
        getattr(eng, method)(**kw)
    text = str(ei.value)
    assert text.startswith(method + ":") and arg in text, text


@pytest.mark.parametrize("method", list(METHODS))
def test_well_formed_arguments_reach_the_library(method):
    """the good arguments above pass every check: the first thing to fail is the missing library"""
    eng = Engine.__new__(Engine)
    kw = {k: v for k, v in good_args().items() if k in METHODS[method]}
    with pytest.raises(AttributeError):
        getattr(eng, method)(**kw)


def test_every_array_argument_of_every_method_is_covered():
    import inspect
    scalars = {"self", "L", "seed_len", "top_k", "hyper", "snapshot_every", "want_cos", "init_ids"}   # init_ids: one row of any T
    for method, params in METHODS.items():
        names = [p for p in inspect.signature(getattr(Engine, method)).parameters if p not in ("snapshot_every", "want_cos", "self")]
        assert tuple(names) == params, method
        assert all(p in BAD for p in names if p not in scalars), method
