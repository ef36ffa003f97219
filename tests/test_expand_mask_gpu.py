"""expand_mask_rows_kernel and the host tables of czc_fluency_rows (csrc/fluency.hip) through their hook: every output array equals
the NumPy model of tests/fluency_ref.py."""
import numpy as np
import pytest

import fluency_hooks as FH
import fluency_ref as FR

pytestmark = pytest.mark.gpu

PAD, MASK = 0, 103


def _rows(R, T, seed_len, lens, seed):
    rng = np.random.default_rng(seed)
    rows = np.full((R, T), PAD, dtype=np.int32)
    for r in range(R):
        L = T - seed_len - 1 if lens is None else lens[r]
        rows[r, :seed_len + L + 1] = rng.integers(1000, 30000, size=seed_len + L + 1)
    return rows


@pytest.mark.parametrize("seed_len", [1, 4])
@pytest.mark.parametrize("case", ["dense", "ragged", "one_row", "one_word", "many"])
def test_expansion_equals_the_numpy_model(case, seed_len):
    R, T, lens = {"dense": (3, seed_len + 6, None), "ragged": (5, seed_len + 7, [1, 3, 6, 6, 4]), "one_row": (1, seed_len + 5, [3]),
                  "one_word": (4, seed_len + 2, [1, 1, 1, 1]), "many": (70, seed_len + 9, [1 + (r * 5) % 8 for r in range(70)])}[case]
    rows = _rows(R, T, seed_len, lens, seed=R + seed_len)
    if case == "ragged":
        rows[2, seed_len + 1] = MASK     # a [MASK] left in a row is a word like any other: its target is mask_id
    ids, target, gen = FH.expand_mask(rows, seed_len, MASK, lens)
    ref_ids, ref_target, ref_gen = FR.expand_ref(rows, seed_len, lens, MASK)
    assert ids.shape == ref_ids.shape
    np.testing.assert_array_equal(ids, ref_ids)
    np.testing.assert_array_equal(target, ref_target)
    np.testing.assert_array_equal(gen, ref_gen)
    if lens is not None:   # the tails stay [PAD]: nothing behind a row's own tokens is written
        n = 0
        for r in range(R):
            for _ in range(lens[r]):
                assert (ids[n, seed_len + lens[r] + 1:] == PAD).all()
                n += 1
