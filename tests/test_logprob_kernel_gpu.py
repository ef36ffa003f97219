"""logprob_target_kernel (csrc/fluency.hip) through its hook, against the float64 reference of tests/fluency_ref.py: rank exact,
|logp - ref64| <= 5e-6 (fluency_ref.KERNEL_BAR; tests/test_fluency_cpu.py shows plain fp32 arithmetic meets it on these inputs)."""
import numpy as np
import pytest

import fluency_hooks as FH
import fluency_ref as FR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [1, 3, 130])
def test_logp_and_rank_at_every_vocabulary_size(N):
    """Odd V give rows that start off a 16-byte boundary; V < 256 leaves lanes without an element; targets at id 0, id V - 1, the
    row maximum, the row minimum and inside a run of equal values (fluency_ref.kernel_case)."""
    worst = 0.0
    for V in FR.VOCABS:
        for t in FR.TEMPS:
            x, target = FR.kernel_case(N, V, t, seed=V)
            ref, ref_rank = FR.logprob_ref(x, target, t)
            logp, rank, flag = FH.logprob(x, target, t)
            assert flag == 0, (V, t)
            assert (rank == ref_rank).all(), (V, t, rank[rank != ref_rank][:4], ref_rank[rank != ref_rank][:4])
            err = float(np.abs(logp.astype(np.float64) - ref).max())
            worst = max(worst, err)
            assert err <= FR.KERNEL_BAR, (V, t, err)
    print(f"logprob_target_kernel N={N}: worst |logp - ref64| = {worst:.2e}")


def test_planted_infinity_raises_the_flag():
    x, target = FR.kernel_case(3, 1025, 1.0, seed=9)
    x[1, 77] = np.inf
    logp, rank, flag = FH.logprob(x, target, 1.0)
    assert flag == 1 and not np.isfinite(logp[1])
    ref, ref_rank = FR.logprob_ref(np.delete(x, 1, axis=0), np.delete(target, 1), 1.0)   # the other rows are untouched
    assert (np.delete(rank, 1) == ref_rank).all() and np.abs(np.delete(logp, 1) - ref).max() <= FR.KERNEL_BAR
