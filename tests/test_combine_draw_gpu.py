"""-m gpu: the drawing instantiation of the combine kernel (csrc/combine.hip, czc_generate_rows_draw) through the kernel-level
hook czc_test_combine_draw, against the NumPy reference of the draw (tests/draw_ref.py) on the final_score the hook returns.
A draw the reference calls a near tie (gap below 1e-4 * (1 + |z_best|): the device computes z in fp32) is left out of the
comparison; at most 1 % of the draws of a test may be."""
import numpy as np
import pytest

import draw_ref as R
import kernel_hooks as H
from conzic_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _hyper(senti):
    return Engine.hyper(0.1, 2.0, 0.1, 0.5) if senti else Engine.hyper(0.02, 2.0, 0.1)


def _compare(tag, best, final, probs, seeds, tau, step):
    want, tie = R.winners(final, probs, seeds, tau, step)
    bad = (best != want) & ~tie
    print(f"[combine_draw] {tag}: {best.size} draws, {int(tie.sum())} near ties, {int((best != want).sum())} differ from the reference, "
          f"{int(bad.sum())} outside a near tie")
    assert tie.mean() <= R.NEAR_TIE_CAP
    assert not bad.any(), np.nonzero(bad)[0][:8]
    return want


@pytest.mark.parametrize("senti", [False, True])
@pytest.mark.parametrize("B,K", R.COMBINE_CASES)
def test_winners_are_the_reference_draw(B, K, senti):
    """tau in {0.05, 0.5} at steps 0 and 7: the winners are the reference's on the kernel's own final_score; the scores are those
    of czc_test_combine bit for bit; where K > 1 the draw moves some winners off the argmax at tau = 0.5."""
    tf, ie, pr, seeds, sr, rp = R.combine_inputs(B, K, senti)
    hp = _hyper(senti)
    _, _, fs0, best0 = H.combine(tf, ie, R.LOGIT_SCALE, pr, hp, sr, rp)
    for tau in R.COMBINE_TAUS:
        for step in R.COMBINE_STEPS:
            fs, best = R.combine_draw(tf, ie, R.LOGIT_SCALE, pr, hp, R.make_draws(seeds, tau), step, sr, rp)
            np.testing.assert_array_equal(fs.view(np.int32), fs0.view(np.int32))
            assert (best >= 0).all() and (best < K).all()
            _compare(f"B {B} K {K} senti {senti} tau {tau} step {step}", best, fs, pr, seeds, tau, step)
            if K > 1 and B >= 64 and tau == 0.5:
                assert (best != best0).any()
    # step0 adds to the step: (step0 = 3, step 4) is step 7
    fs, best = R.combine_draw(tf, ie, R.LOGIT_SCALE, pr, hp, R.make_draws(seeds, 0.5, step0=3), 4, sr, rp)
    _compare(f"B {B} K {K} step0 3 + 4", best, fs, pr, seeds, 0.5, 7)


def test_tau_zero_rows_keep_the_first_argmax():
    """A mixed array: every third row has tau = 0 and returns the best of czc_test_combine; the others draw."""
    B, K = 64, 200
    tf, ie, pr, seeds, _, _ = R.combine_inputs(B, K)
    hp = _hyper(False)
    pr[5] = pr[5, 0]                # a row of equal fluency ...
    tf[5 * K:(5 + 1) * K] = tf[5 * K]   # ... and equal features: all K scores tie, the first index wins
    taus = np.where(np.arange(B) % 3 == 0, 0.0, 0.5).astype(np.float32)
    taus[5] = 0.0
    _, _, fs0, best0 = H.combine(tf, ie, R.LOGIT_SCALE, pr, hp)
    fs, best = R.combine_draw(tf, ie, R.LOGIT_SCALE, pr, hp, R.make_draws(seeds, taus), 2)
    np.testing.assert_array_equal(fs.view(np.int32), fs0.view(np.int32))
    np.testing.assert_array_equal(best[taus == 0], best0[taus == 0])
    assert best[5] == 0
    _compare("mixed tau", best, fs, pr, seeds, taus, 2)
    assert (best[taus > 0] != best0[taus > 0]).any()


def test_zero_probability_candidates_are_never_drawn():
    """tau = 1e6 (the scores no longer matter): winners spread over the eligible candidates only; a row without any eligible
    candidate falls back to the first argmax."""
    B, K = 256, 8
    tf, ie, pr, seeds, _, _ = R.combine_inputs(B, K)
    hp = _hyper(False)
    pr[:, [1, 4, 6]] = 0.0
    pr[7] = 0.0                      # no eligible candidate
    _, _, _, best0 = H.combine(tf, ie, R.LOGIT_SCALE, pr, hp)
    fs, best = R.combine_draw(tf, ie, R.LOGIT_SCALE, pr, hp, R.make_draws(seeds, 1e6), 0)
    _compare("tau 1e6", best, fs, pr, seeds, 1e6, 0)
    rows = np.arange(B) != 7
    assert not np.isin(best[rows], [1, 4, 6]).any()
    assert set(best[rows].tolist()) == {0, 2, 3, 5, 7}
    assert best[7] == best0[7]


def test_permuting_the_rows_permutes_the_winners():
    B, K = 64, 200
    tf, ie, pr, seeds, _, _ = R.combine_inputs(B, K)
    hp = _hyper(False)
    _, best = R.combine_draw(tf, ie, R.LOGIT_SCALE, pr, hp, R.make_draws(seeds, 0.5), 3)
    perm = np.random.default_rng(9).permutation(B)
    tfp = tf.reshape(B, K, -1)[perm].reshape(B * K, -1)
    _, bestp = R.combine_draw(tfp, ie[perm], R.LOGIT_SCALE, pr[perm], hp, R.make_draws(seeds[perm], 0.5), 3)
    np.testing.assert_array_equal(bestp, best[perm])
