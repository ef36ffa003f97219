"""The step memo's rule on the host (conzic_amd/harness.py::memo_expected_hits, option "memo" of czc_generate): hand-built
trajectories whose hits are known by construction.  No GPU."""
import numpy as np

from conzic_amd import harness

MASK, SEED, T = 103, 2, 8   # [CLS] w [words x 4] ... : positions 0..3 are columns 2..5


def _traj(rows_after):
    """int32 [n_steps, B, T] from a list of per-step lists of rows (each row a list of T ids)."""
    return np.asarray(rows_after, dtype=np.int32)


def _row(words):
    return [101, 7] + list(words) + [1012, 102]


def _run_order(order, rows_by_sweep, B=1):
    """Snapshots of B identical images: rows_by_sweep[sweep][i] = the words after the i-th step of that sweep."""
    snaps = []
    for sweep in rows_by_sweep:
        for words in sweep:
            snaps.append([_row(words)] * B)
    return _traj(snaps)


def test_sequential_fixed_point_in_sweep_two_hits_from_sweep_three():
    L = 4
    pos = list(range(L)) * 5
    # sweep 1 fills the masks; sweep 2 changes position 0 and from then on every row stays: the fixed point is reached in
    # sweep 2, so every step of sweep 3 and later sees the masked row its position saw in the sweep before
    s1 = [[10, MASK, MASK, MASK], [10, 11, MASK, MASK], [10, 11, 12, MASK], [10, 11, 12, 13]]
    fixed = [[20, 11, 12, 13]] * L
    snaps = _run_order("sequential", [s1, fixed, fixed, fixed, fixed], B=3)
    hits = harness.memo_expected_hits(snaps, pos, None, SEED, MASK)
    assert hits.shape == (20, 3)
    assert not hits[:8].any()          # sweep 1 is a first visit; every sweep-2 step sees a fuller row than in sweep 1
    assert hits[8:].all()


def test_sequential_visit_after_a_late_change_misses():
    """Sweep 2 changes position 2 AFTER position 0's visit: position 0's sweep-3 masked row differs from its sweep-2 one."""
    L = 4
    pos = list(range(L)) * 4
    s1 = [[10, MASK, MASK, MASK], [10, 11, MASK, MASK], [10, 11, 12, MASK], [10, 11, 12, 13]]
    s2 = [[10, 11, 12, 13], [10, 11, 12, 13], [10, 11, 22, 13], [10, 11, 22, 13]]
    fixed = [[10, 11, 22, 13]] * L
    hits = harness.memo_expected_hits(_run_order("sequential", [s1, s2, fixed, fixed]), pos, None, SEED, MASK)[:, 0]
    # sweep 3: positions 0 and 1 saw [.. 12 ..] in sweep 2 and see [.. 22 ..] now; positions 2 and 3 saw 22 already
    assert hits[8:12].tolist() == [False, False, True, True]
    assert hits[12:].all()


def test_shuffle_order_keys_by_position():
    order = [2, 0, 3, 1]
    pos = order * 3
    cur = [MASK] * 4
    snaps = []
    words = {0: 30, 1: 31, 2: 32, 3: 33}
    for p in order:          # sweep 1 fills in shuffle order
        cur = list(cur)
        cur[p] = words[p]
        snaps.append([_row(cur)])
    for _ in range(2):       # fixed point from then on
        for p in order:
            snaps.append([_row(cur)])
    hits = harness.memo_expected_hits(_traj(snaps), pos, None, SEED, MASK)[:, 0]
    # sweep 2: position 2 saw [M M M M] in sweep 1 and sees [30 31 M 33] now: a miss, and so do 0 and 3; position 1 was the
    # last one sweep 1 filled, so it sees [30 M 32 33] both times: a hit in the first revisit already
    assert hits[:8].tolist() == [False] * 7 + [True]
    assert hits[8:].all()


def test_span_zero_step_hits_with_its_two_step():
    """Span order (n_mask 2 then 0): the n_mask = 0 step hits exactly when the n_mask = 2 step of its group hit."""
    pos = [0, 1, 2, 3] * 3
    nm = [2, 0, 2, 0] * 3
    A, B_ = [40, 41, 42, 43], [50, 41, 52, 53]
    snaps = [
        # sweep 1, both images: (0, 2) writes 40 and leaves position 1 masked, (1, 0) writes 41, then (2, 2) / (3, 0)
        [_row([40, MASK, MASK, MASK])] * 2, [_row([40, 41, MASK, MASK])] * 2,
        [_row([40, 41, 42, MASK])] * 2, [_row(A)] * 2,
        # sweep 2: image 0 stays; image 1 moves at position 0, hence at position 2
        [_row(A), _row([50, MASK, 42, 43])], [_row(A), _row([50, 41, 42, 43])],
        [_row(A), _row([50, 41, 52, MASK])], [_row(A), _row(B_)],
        # sweep 3: image 1's group (0, 2) sees [M M 52 53] instead of [M M 42 43] (and keeps its words); its group (2, 2) then
        # sees [50 41 M M] as in sweep 2
        [_row(A), _row([50, MASK, 52, 53])], [_row(A), _row(B_)],
        [_row(A), _row([50, 41, 52, MASK])], [_row(A), _row(B_)],
    ]
    hits = harness.memo_expected_hits(_traj(snaps), pos, nm, SEED, MASK)
    assert hits[:4].sum() == 0
    assert hits[4].tolist() == [False, False]      # [M M 42 43] vs sweep 1's [M M M M]
    assert hits[6].tolist() == [True, False]       # image 0: [40 41 M M] both times; image 1: [50 41 M M] vs [40 41 M M]
    assert hits[8].tolist() == [True, False]
    assert hits[10].tolist() == [True, True]
    for s in (1, 3, 5, 7, 9, 11):                  # the zero steps go with their two-step
        assert (hits[s] == hits[s - 1]).all()


def test_random_order_with_repeated_positions():
    pos = [1, 1, 3, 0, 1, 3, 3, 2]
    cur = [MASK] * 4
    snaps = []
    # every position writes 60 + position, once filled a row never changes
    for p in pos:
        cur = list(cur)
        cur[p] = 60 + p
        snaps.append([_row(cur)])
    hits = harness.memo_expected_hits(_traj(snaps), pos, [1] * len(pos), SEED, MASK)[:, 0]
    # step 1 (pos 1 again, nothing else changed since step 0): hit; step 4 (pos 1): positions 3 and 0 were filled in between:
    # miss; step 5 (pos 3): position 0 was still masked at step 2: miss; step 6 (pos 3 again right after step 5): hit
    assert hits.tolist() == [False, True, False, False, False, False, True, False]


def test_changed_row_elsewhere_misses_and_never_steps_do_not_hit():
    L = 2
    pos = [0, 1] * 4
    # position 0 moves at its second visit (75), which moves position 1 at its next visit (72); then a fixed point
    rows = [[70, MASK], [70, 71], [75, 71], [75, 72], [75, 72], [75, 72], [75, 72], [75, 72]]
    snaps = _traj([[_row(r)] for r in rows])
    hits = harness.memo_expected_hits(snaps, pos, None, SEED, MASK)[:, 0]
    # step 2 (pos 0): [M 71] vs [M M]; step 3 (pos 1): [75 M] vs [70 M]; step 4 (pos 0): [M 72] vs [M 71] -- each a row that
    # changed at the other position since the last visit; steps 5-7 see their last visit's row again
    assert hits.tolist() == [False, False, False, False, False, True, True, True]
    never = harness.memo_refine_no_hit(len(pos), snapshot_every=1, want_cos=True)
    assert never.all()   # REFINE with every step's cosine returned: nothing may hit
    assert not harness.memo_expected_hits(snaps, pos, None, SEED, MASK, never=never).any()
    never2 = harness.memo_refine_no_hit(len(pos), snapshot_every=2, want_cos=False)
    assert never2.tolist() == [False, True, False, False, False, False, False, False]   # only the audit step of sweep 1


def test_memo_groups():
    assert harness.memo_groups([2, 0, 2, 0, 1], 5) == [(0, 2), (2, 2), (4, 1)]
    assert harness.memo_groups(None, 3) == [(0, 1), (1, 1), (2, 1)]
