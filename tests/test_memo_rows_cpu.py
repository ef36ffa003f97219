"""The rows memo's rule on the host (conzic_amd/harness.py::memo_expected_hits_rows, option "memo_rows" of czc_generate_rows)
against the step memo's (memo_expected_hits) on trajectories of a toy polishing rule, and the CZC_MEMO_ROWS switch.  No GPU."""
import numpy as np
import pytest

from conzic_amd import harness, runtime

MASK, SEED, L = 103, 2, 6
T = SEED + L + 2


def _winner(p, masked, target):
    """A deterministic function of the masked row, as the polishing rule is: the row's target word once the word to the left
    is its target (position 0: at once), else the target + 1.  The visiting order decides how fast a row settles: left to
    right in one sweep, right to left one position per sweep."""
    left_ok = p == 0 or masked[SEED + p - 1] == target[p - 1]
    return int(target[p]) + (0 if left_ok else 1)


def _simulate(positions, n_mask, targets):
    """Snapshots int32 [n_steps, R, T] of R rows under positions [n_steps, R]: n_mask >= 1 masks that many columns and writes
    the winner at the first; n_mask = 0 writes the winner of its own position from the masked row of the step before."""
    positions = np.asarray(positions)
    n_steps, R = positions.shape
    cur = np.full((R, T), 7, np.int32)
    cur[:, SEED:SEED + L] = MASK
    seen = [None] * R
    snaps = np.empty((n_steps, R, T), np.int32)
    for s in range(n_steps):
        for r in range(R):
            p = int(positions[s, r])
            if n_mask[s] >= 1:
                cur[r, SEED + p:SEED + p + n_mask[s]] = MASK
                seen[r] = cur[r].copy()
            cur[r, SEED + p] = _winner(p, seen[r], targets[r])
        snaps[s] = cur
    return snaps


def _targets(R):
    return np.random.default_rng(3).integers(1000, 2000, size=(R, L)) * 2   # even: target + 1 is never another target


@pytest.mark.parametrize("order", ["sequential", "shuffle", "span"])
def test_same_order_in_every_row_is_the_step_memo_rule(order):
    R, sweeps = 5, 5
    pos, nm, _ = harness.order_positions(order, L, sweeps, order_list=[4, 1, 5, 0, 3, 2])
    rows = np.repeat(np.array(pos)[:, None], R, axis=1)
    snaps = _simulate(rows, nm, _targets(R))
    want = harness.memo_expected_hits(snaps, pos, nm, SEED, MASK)
    got = harness.memo_expected_hits_rows(snaps, rows, nm, SEED, MASK)
    assert got.shape == (len(pos), R) and got.dtype == bool
    np.testing.assert_array_equal(got, want)
    assert want.any() and not want.all()
    never = harness.memo_refine_no_hit(len(pos), L, want_cos=True)
    np.testing.assert_array_equal(harness.memo_expected_hits_rows(snaps, rows, nm, SEED, MASK, never=never),
                                  harness.memo_expected_hits(snaps, pos, nm, SEED, MASK, never=never))


def _mixed(R, sweeps):
    rng = np.random.default_rng(9)
    orders = [list(range(L)), list(range(L))[::-1]] + [list(rng.permutation(L)) for _ in range(R - 2)]
    cols = [harness.order_positions("shuffle", L, sweeps, order_list=o)[0] for o in orders]
    return np.array(cols, dtype=np.int32).T, [1] * (L * sweeps)


def test_rows_with_different_orders_are_one_step_memo_rule_per_order():
    R, sweeps = 6, 8
    rows, nm = _mixed(R, sweeps)
    snaps = _simulate(rows, nm, _targets(R))
    got = harness.memo_expected_hits_rows(snaps, rows, nm, SEED, MASK)
    for r in range(R):
        want = harness.memo_expected_hits(snaps[:, r:r + 1], rows[:, r].tolist(), nm, SEED, MASK)[:, 0]
        np.testing.assert_array_equal(got[:, r], want, err_msg=f"row {r}")
    first_hit = [int(np.argmax(got[:, r])) for r in range(R)]
    assert got.all(axis=0).sum() == 0 and got[-L:].all()   # every row settles, none hits from the start
    assert len(set(first_hit)) > 1                            # and they settle at different times: a compact batch on the way


def test_one_changed_token_loses_exactly_the_hits_that_depend_on_it():
    R, sweeps = 4, 6
    rows, nm = _mixed(R, sweeps)
    snaps = _simulate(rows, nm, _targets(R))
    base = harness.memo_expected_hits_rows(snaps, rows, nm, SEED, MASK)
    r, s = 2, 4 * L + 1                       # a late step of row 2, inside its run of hits
    p = int(rows[s, r])
    later = [t for t in range(s + 1, len(nm)) if rows[t, r] == p]
    assert base[s, r] and base[later[0], r]
    mut = snaps.copy()
    col = SEED + (p + 1) % L                  # a column the step did not mask: part of the compared row
    mut[s, r, col] += 1                       # (one snapshot only: the rows before and after are the trajectory's)
    got = harness.memo_expected_hits_rows(mut, rows, nm, SEED, MASK)
    lost = {tuple(x) for x in np.argwhere(base & ~got)}
    # the visit at s no longer sees its entry's row, and the next visit of that position no longer sees the row s recorded
    assert lost == {(s, r), (later[0], r)}
    assert not (got & ~base).any()
    # the changed token inside the step's own masked column is not part of the key: nothing is lost
    mut2 = snaps.copy()
    mut2[s, r, SEED + p] += 1
    np.testing.assert_array_equal(harness.memo_expected_hits_rows(mut2, rows, nm, SEED, MASK), base)


def test_another_group_shape_at_the_same_first_position_replaces_the_entry():
    """The slot is (row, first position): position 0 visited as a one-step group, then as the head of a span, then as a
    one-step group again.  The step memo keeps one entry per key and hits; the rows memo's slot was replaced."""
    pos, nm = [0, 0, 0, 1, 0, 0], [1, 1, 2, 0, 1, 1]
    snaps = np.full((len(pos), 1, T), 7, np.int32)
    rows = np.array(pos)[:, None]
    assert harness.memo_expected_hits(snaps, pos, nm, SEED, MASK)[:, 0].tolist() == [False, True, False, False, True, True]
    assert harness.memo_expected_hits_rows(snaps, rows, nm, SEED, MASK)[:, 0].tolist() == [False, True, False, False, False, True]


def test_groups_that_never_hit():
    pos, nm = [0, 1, 2, 0, 1, 2], [3, 0, 0, 3, 0, 0]   # three steps per group: more than an entry holds
    snaps = np.full((len(pos), 2, T), 7, np.int32)
    assert not harness.memo_expected_hits_rows(snaps, np.repeat(np.array(pos)[:, None], 2, axis=1), nm, SEED, MASK).any()
    pos, nm = [1, 0, 1, 0, 1], [0, 2, 0, 2, 0]         # the call starts inside a group
    snaps = np.full((len(pos), 1, T), 7, np.int32)
    assert harness.memo_expected_hits_rows(snaps, np.array(pos)[:, None], nm, SEED, MASK)[:, 0].tolist() == [False, False, False, True, True]


def test_czc_memo_rows_env(monkeypatch):
    monkeypatch.delenv("CZC_MEMO_ROWS", raising=False)
    assert runtime.memo_rows_setting() == 0
    for v, want in (("0", 0), ("1", 1), ("on", 1), ("off", 0), (" True ", 1), ("no", 0), ("", 0)):
        monkeypatch.setenv("CZC_MEMO_ROWS", v)
        assert runtime.memo_rows_setting() == want
    monkeypatch.setenv("CZC_MEMO_ROWS", "2")
    with pytest.raises(ValueError, match="CZC_MEMO_ROWS"):
        runtime.memo_rows_setting()
    monkeypatch.setenv("CZC_MEMO", "1")            # the two switches are independent
    monkeypatch.setenv("CZC_MEMO_ROWS", "0")
    assert runtime.memo_setting() == 1 and runtime.memo_rows_setting() == 0
