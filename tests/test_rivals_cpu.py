"""Rival images (czc_generate_rows_vs): the library's symbols, conzic_amd/rivals.py and the command-line refusals.  No GPU."""
import numpy as np
import pytest

from conzic_amd import native, rivals
from conzic_amd.demo_cli import get_args


def test_library_exports_the_calls_and_the_version():
    lib = native.load()
    assert lib.czc_version() >= 106
    assert hasattr(lib, "czc_generate_rows_vs") and hasattr(lib, "czc_score_rows_vs")
    assert "czc_generate_rows_vs" in native.SIGNATURES and "czc_score_rows_vs" in native.SIGNATURES
    assert "czc_test_combine_rivals" in native.TEST_SIGNATURES
    assert hasattr(native.load_test(), "czc_test_combine_rivals")
    with open(native.HEADER_PATH) as f:
        hdr = f.read()
    assert "#define CZC_MAX_RIVALS 16" in hdr and native.MAX_RIVALS == rivals.MAX_RIVALS == 16
    for must in ("czc_generate_rows_tied itself, bit for bit", "uploaded once, with the schedule", "CZC_PREC_REFINE", "CZC_ERR_STATE",
                 "a filled slot behind an empty one", "a rival equal to the row's own image", "Either output pointer may be NULL"):
        assert must in hdr, must


def _unit(vecs):
    v = np.asarray(vecs, dtype=np.float64)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def test_rival_table_lists_the_nearest_others():
    rng = np.random.default_rng(0)
    emb = rng.standard_normal((7, 16)).astype(np.float32)
    tab = rivals.rival_table(emb, 3)
    assert tab.shape == (7, 3) and tab.dtype == np.int32
    en = _unit(emb)
    cos = en @ en.T
    for b in range(7):
        assert b not in tab[b]
        others = sorted((j for j in range(7) if j != b), key=lambda j: (-cos[b, j], j))
        assert tab[b].tolist() == others[:3]
    # scaling an embedding changes nothing: the table is built on cosines
    np.testing.assert_array_equal(rivals.rival_table(emb * np.float32(3.0), 3), tab)


def test_rival_table_breaks_ties_by_the_lowest_index():
    e = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0], [0.0, 1.0], [1.0, 0.0]])
    tab = rivals.rival_table(e, 2)
    assert tab[0].tolist() == [4, 1]          # image 4 is a copy; 1, 2, 3 tie at cosine 0: the lowest
    assert tab[1].tolist() == [2, 3]
    assert tab[3].tolist() == [1, 2]


def test_rival_table_sets_and_short_sets():
    rng = np.random.default_rng(1)
    emb = rng.standard_normal((6, 8))
    tab = rivals.rival_table(emb, 3, sets=[0, 0, 1, 1, 1, 2])
    assert set(tab[0].tolist()) == {1, -1} and tab[0, 0] == 1 and tab[0, 1:].tolist() == [-1, -1]
    assert sorted(tab[2][:2].tolist()) == [3, 4] and tab[2, 2] == -1
    assert tab[5].tolist() == [-1, -1, -1]      # a set of one: no rival
    whole = rivals.rival_table(emb[:3], 4)
    assert (whole[:, 2:] == -1).all() and (whole[:, :2] >= 0).all()
    for bad_m in (0, 17):
        with pytest.raises(ValueError):
            rivals.rival_table(emb, bad_m)
    with pytest.raises(ValueError):
        rivals.rival_table(np.zeros((2, 4)), 1)


def test_expand_maps_the_table_to_rows():
    tab = np.array([[1, 2], [0, -1], [0, 1]], dtype=np.int32)
    rows = rivals.expand(tab, [2, 0, 0, 1])
    assert rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"]
    assert rows.tolist() == [[0, 1], [1, 2], [1, 2], [0, -1]]
    with pytest.raises(ValueError):
        rivals.expand(tab, [3])
    rivals.check_table(rows, [2, 0, 0, 1], 3)
    for bad in ([[2, 1]], [[-1, 1]], [[3, -1]], [[-2, -1]]):
        with pytest.raises(ValueError):
            rivals.check_table(np.array(bad), [2], 3)


def test_disc_ref_is_stable_and_exact_where_it_can_be():
    s = 100.0
    # cosine gaps of +-2 at exp(logit_scale) = 100: exponents of +-200, no overflow, no NaN
    d = rivals.disc_ref(np.array([1.0, -1.0]), np.array([[-1.0, -1.0], [1.0, 1.0]]), s)
    assert np.isfinite(d).all() and d[0] == 1.0 and 0.0 <= d[1] < 1e-80
    for m in (1, 3, 16):
        np.testing.assert_allclose(rivals.disc_ref(np.full(4, 0.3), np.full((4, m), 0.3), s), 1.0 / (m + 1), rtol=1e-15)
    # empty slots do not count
    c0, cj = np.array([0.2]), np.array([[0.25, 0.9, 0.1]])
    only = rivals.disc_ref(c0, cj, s, valid=[[True, False, True]])
    np.testing.assert_allclose(only, rivals.disc_ref(c0, cj[:, [0, 2]], s), rtol=1e-15)
    assert rivals.disc_ref(c0, cj, s, valid=[[False, False, False]])[0] == 1.0
    # against the plain softmax over the images
    lg = s * np.array([0.2, 0.25, 0.9, 0.1])
    np.testing.assert_allclose(rivals.disc_ref(c0, cj, s)[0], np.exp(lg[0] - lg.max()) / np.exp(lg - lg.max()).sum(), rtol=1e-12)


@pytest.mark.parametrize("argv", [
    ["--distinct", "1.0", "--sentence_lens", "4,6"],
    ["--distinct", "1.0", "--signals", "caption,positive"],
    ["--distinct", "1.0", "--block_width", "2", "--order", "sequential"],
    ["--distinct", "1.0", "--run_type", "infill", "--caption", "a _ dog", "--order", "sequential"],
    ["--distinct", "1.0", "--run_type", "retrieve", "--index_captions", "x.txt"],
    ["--distinct", "nan"],
    ["--distinct", "inf"],
    ["--distinct", "1.0", "--distinct_rivals", "0"],
    ["--distinct", "1.0", "--distinct_rivals", "17"],
    ["--rival_images", "a.jpg"],
])
def test_cli_refusals(argv, capsys):
    with pytest.raises(SystemExit) as ei:
        get_args(["--synthetic"] + argv)
    assert ei.value.code == 2
    err = capsys.readouterr().err
    assert "--distinct" in err or "--rival_images" in err


def test_cli_accepts_the_combinations_it_serves():
    a = get_args(["--synthetic", "--distinct", "1.5", "--batch_samples", "--sample_tau", "0.5"])
    assert a.distinct == 1.5 and a.distinct_rivals == 4 and a.rival_images is None
    a = get_args(["--synthetic", "--distinct", "-0.5", "--distinct_rivals", "16", "--run_type", "controllable",
                  "--rival_images", "a.jpg, b.jpg"])
    assert a.rival_images == ["a.jpg", "b.jpg"] and a.distinct == -0.5
    assert get_args(["--synthetic"]).distinct == 0.0
