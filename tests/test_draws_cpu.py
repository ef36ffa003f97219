"""CPU: the NumPy reference of the seeded draw (tests/draw_ref.py: Philox4x32-10, the uniform, the Gumbel-max rule), the seeds
of conzic_amd/draws.py, conzic_amd/diversity.py and the --sample_tau plumbing of the CLIs.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import draw_ref as R
from conzic_amd import demo_cli, diversity, draws, native
from conzic_amd.engine import draw_array

SEED_BASE = 20261019   # of the distribution checks below: picked once, kept


def test_philox_known_answer():
    assert [int(v) for v in R.philox4x32_10([0, 0, 0, 0], [0, 0])] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    # Random123's other two vectors of philox4x32-10: all ones, and the digits of pi
    ones = [0xffffffff] * 4
    assert [int(v) for v in R.philox4x32_10(ones, ones[:2])] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    pi = R.philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])
    assert [int(v) for v in pi] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # words(): candidate k reads word k & 3 of the block with counter (step, k >> 2, 0, 0) under key (seed lo, seed hi)
    seed, step = 0x0123456789abcdef, 5
    x = R.words(seed, step, 11)
    for k in (0, 3, 4, 10):
        blk = R.philox4x32_10([step, k >> 2, 0, 0], [seed & 0xffffffff, seed >> 32])
        assert int(x[k]) == int(blk[k & 3])


def test_uniform_is_an_fp32_number_strictly_inside_the_unit_interval():
    u = R.uniform(np.array([0, 0x1ff, 0x200, 0x7fffffff, 0xffffffff], dtype=np.uint32))
    assert (u > 0).all() and (u < 1).all()
    np.testing.assert_array_equal(u.astype(np.float32).astype(np.float64), u)
    assert u[0] == 2.0 ** -24 and u[-1] == 1.0 - 2.0 ** -24
    assert np.float32(u[-1]) < np.float32(1.0) and np.isfinite(R.gumbel(np.array([0, 0xffffffff], dtype=np.uint32))).all()


def _chi2(counts, p):
    n = counts.sum()
    return float(((counts - n * p) ** 2 / (n * p)).sum())


def test_winners_follow_softmax_of_final_over_tau():
    """K = 8 fixed scores, 4096 seeds, tau = 0.5: Pearson's statistic against softmax(final / tau) stays below 24.32, the 0.999
    quantile of chi-square with 7 degrees of freedom (the seeds are fixed: deterministic)."""
    final = np.array([0.9, 0.1, 0.5, 1.2, 0.3, 0.7, 0.0, 1.0])
    n, tau = 4096, 0.5
    seeds = np.array([draws.row_seed(SEED_BASE, 1, i) for i in range(n)], dtype=np.uint64)
    win, _ = R.winners(np.tile(final, (n, 1)), np.ones((n, 8)), seeds, tau, 3)
    p = np.exp(final / tau)
    p /= p.sum()
    stat = _chi2(np.bincount(win, minlength=8).astype(np.float64), p)
    print(f"chi-square {stat:.2f}")
    assert stat < 24.32


def test_large_tau_is_uniform_over_the_eligible_candidates():
    final = np.array([0.9, 0.1, 0.5, 1.2, 0.3, 0.7, 0.0, 1.0])
    probs = np.array([1, 0, 1, 1, 0, 1, 0, 1], dtype=np.float32)
    n = 4096
    seeds = np.array([draws.row_seed(SEED_BASE, 2, i) for i in range(n)], dtype=np.uint64)
    win, _ = R.winners(np.tile(final, (n, 1)), np.tile(probs, (n, 1)), seeds, 1e6, 0)
    counts = np.bincount(win, minlength=8).astype(np.float64)
    assert counts[probs == 0].sum() == 0                       # never drawn
    stat = _chi2(counts[probs > 0], np.full(5, 0.2))
    print(f"chi-square {stat:.2f}")
    assert stat < 18.47                                        # 0.999 quantile, 4 degrees of freedom


def test_rows_without_an_eligible_candidate_and_tau_zero_rows_take_the_first_argmax():
    final = np.array([[0.2, 0.9, 0.9, 0.1], [0.5, 0.1, 0.7, 0.7]])
    win, tie = R.winners(final, np.zeros((2, 4)), [1, 2], 0.5, 0)
    assert win.tolist() == [1, 2] and not tie.any()
    win, tie = R.winners(final, np.ones((2, 4)), [1, 2], [0.0, 0.0], 0)
    assert win.tolist() == [1, 2] and not tie.any()


def test_near_tie_share_of_the_gpu_tests_inputs():
    """The reference's own share of near ties on the exact inputs tests/test_combine_draw_gpu.py uses (float64 scores here, the
    kernel's fp32 ones there) is within the cap the GPU tests hold it to."""
    for B, K in R.COMBINE_CASES:
        for senti in (False, True):
            tf, ie, pr, seeds, sr, rp = R.combine_inputs(B, K, senti)
            f = R.fused_ref(tf, ie, pr, 0.1 if senti else 0.02, 2.0, sr, rp, 0.5)
            for tau in R.COMBINE_TAUS:
                for step in R.COMBINE_STEPS:
                    _, tie = R.winners(f, pr, seeds, tau, step)
                    assert tie.mean() <= R.NEAR_TIE_CAP, (B, K, senti, tau, step, tie.mean())


def test_row_seed_is_distinct_and_stable():
    seeds = {draws.row_seed(42, draws.image_key(f"img{i}.jpg"), s) for i in range(256) for s in range(16)}
    assert len(seeds) == 4096
    assert draws.splitmix64(0) == 0xe220a8397b1dcdaf                       # the generator's first output from state 0
    assert draws.row_seed(42, 7, 3) == 0x0bc8f279ec388fb4
    assert draws.row_seed(42, 7, 3, 1) != draws.row_seed(42, 7, 3)
    assert draws.row_seed(42, draws.image_key("img0"), 0) == draws.row_seed(42, draws.image_key("img0"), 0, 0)
    assert draws.row_seed(0, draws.image_key("img0"), 0) == 0x9c8d62d4dbe684f4   # a name goes through CRC-32: stable across processes


def test_draw_builders():
    rows = draws.sample_rows(42, [1, 2], 3, 0.5, columns=2, step0=4)
    assert len(rows) == 12 and all(isinstance(d, native.Draw) for d in rows)
    assert rows[(1 * 3 + 2) * 2 + 1].seed == draws.row_seed(42, 2, 2, 1) and rows[0].step0 == 4 and rows[0].tau == 0.5
    # a serial loop's call for sample 2 alone gives the row the batched call's seed
    alone = draws.sample_rows(42, [1, 2], 1, 0.5, sample0=2)
    assert [d.seed for d in alone] == [rows[(0 * 3 + 2) * 2 + b].seed for b in range(2)]
    assert draws.sample_rows(42, [1, 2], 3, 0.0) is None
    arr = draw_array(draws.draw_rows([5, 6, 2 ** 64 - 1], [0.0, 0.5, 1.0], step0=7))
    assert C.sizeof(native.Draw) == 16 and len(arr) == 3
    assert [(a.seed, a.tau, a.step0) for a in arr] == [(5, 0.0, 7), (6, 0.5, 7), (2 ** 64 - 1, 1.0, 7)]
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            draws.make_draw(1, bad)
    with pytest.raises(ValueError):
        draws.make_draw(1, 0.5, step0=2 ** 32)
    with pytest.raises(TypeError):
        draw_array([object()])
    assert draws.describe(None) == "" and draws.describe(rows[:2]).startswith(" sample_tau 0.5 seeds [0x")


def test_distinct_n_on_a_hand_computed_example():
    # unigrams: a b a | a c -> 5 tokens, 3 distinct; bigrams: (a b) (b a) | (a c) -> 3, all distinct
    d = diversity.distinct_n(["A b a", "a c"])
    assert d == {1: 3 / 5, 2: 1.0}
    assert diversity.distinct_n(["a b", "a b"]) == {1: 0.5, 2: 0.5}
    assert diversity.distinct_n([""]) == {1: 0.0, 2: 0.0}
    assert diversity.distinct_n(["a"], ns=(2,)) == {2: 0.0}


def test_library_binding_of_generate_rows_draw():
    lib = native.load()
    assert lib.czc_version() >= 104
    fn = lib.czc_generate_rows_draw
    assert len(fn.argtypes) == len(lib.czc_generate_rows_hp.argtypes) + 1
    # a NULL engine is refused before anything is read
    assert fn(None, 2, 8, 4, None, None, None, 8, 0, None, None, 1, None, draw_array(draws.draw_rows([1, 2], 0.5)), None, None) == native.ERR_ARG
    hdr = open(native.HEADER_PATH).read()
    assert "typedef struct czc_draw" in hdr and "uint64_t seed;" in hdr
    assert "czc_test_combine_draw" in native.TEST_SIGNATURES


def test_cli_arguments():
    a = demo_cli.get_args(["--synthetic"])
    assert a.sample_tau == 0.0                                  # off by default
    a = demo_cli.get_args(["--synthetic", "--sample_tau", "0.5", "--batch_samples", "--sentence_lens", "4,6", "--signals", "caption,positive",
                           "--order", "sequential"])
    assert a.sample_tau == 0.5 and a.batch_samples and a.sentence_lens == [4, 6] and a.signals == ["caption", "positive"]
    a = demo_cli.get_args(["--synthetic", "--run_type", "infill", "--caption", "a _ dog", "--order", "sequential", "--sample_tau", "2"])
    assert a.sample_tau == 2.0
    for bad in (["--sample_tau", "-1"], ["--sample_tau", "nan"], ["--sample_tau", "inf"],
                ["--sample_tau", "0.5", "--run_type", "retrieve", "--index_captions", "x.txt"]):
        with pytest.raises(SystemExit):
            demo_cli.get_args(["--synthetic"] + bad)
    from conzic_amd import run_cli
    assert run_cli.get_args is demo_cli.get_args
    import inspect
    from conzic_amd import runtime
    for fn in (runtime.run_generation_samples, runtime.run_generation_lengths, runtime.run_generation_signals):
        assert inspect.signature(fn).parameters["sample_tau"].default == 0.0
