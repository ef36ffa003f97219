"""How EngineGroup deals the rows of a generate_rows* call over its members, checked on fake members that record what they are
handed (no GPU, no library): the parts, every per-row argument's slices, the images in each of the three hand-out modes, the
snapshot interval, and where the results land."""
import inspect

import numpy as np
import pytest

from conzic_amd import native
from conzic_amd.engine import Engine, EngineGroup

R, T, N_STEPS, SEED_LEN, TOP_K, N_IMG, D = 7, 12, 12, 4, 8, 3, 4
GROUPS = np.array([5, 5, 0, 0, 0, 3, 3])        # sizes 2, 3, 2; the ids are not dense
IMAGE_OF_ROW = np.array([2, 2, 0, 0, 0, 1, 1])  # one image per group
LENS = np.array([2, 2, 3, 3, 3, 6, 6])          # one length per group; the longest sits in the last part only
EMBEDS = np.arange(N_IMG * D, dtype=np.float32).reshape(N_IMG, D) + 1.0
INIT = (np.arange(R * T, dtype=np.int32).reshape(R, T) % 50) + 1
POS = np.arange(N_STEPS * R, dtype=np.int32).reshape(N_STEPS, R)   # pos[0, r] = r: a member's columns name its global rows
HYPERS = [Engine.hyper(0.02, 2.0, 0.1 + r) for r in range(R)]
DRAWS = [native.Draw(100 + r, 0.0, r) for r in range(R)]
RIVALS = np.array([[(IMAGE_OF_ROW[r] + 1) % N_IMG, -1] for r in range(R)], np.int32)
DELTAS = np.linspace(0.5, 2.0, R).astype(np.float32)
N_MASK = [1] * N_STEPS


class FakeMember:
    """Stands in for an Engine: records (method, arguments by name) of every call; a generate_rows* call returns ids and cos
    whose values are the member-local row index (plus the snapshot index in the hundreds)."""

    def __init__(self):
        self.calls = []

    def set_image_embeds(self, embeds):
        self.calls.append(("set_image_embeds", dict(embeds=np.array(embeds))))


def _recorder(name):
    sig = inspect.signature(getattr(Engine, name))

    def method(self, *args, **kwargs):
        bound = sig.bind(self, *args, **kwargs)
        bound.apply_defaults()
        a = {k: v for k, v in bound.arguments.items() if k != "self"}
        self.calls.append((name, a))
        pos = np.asarray(a["positions"])
        n_steps, rows = pos.shape
        width = np.asarray(a["init_ids"]).size if "init_ids" in a else np.asarray(a["init_rows"]).shape[1]
        lens = a.get("lens")
        every = a["snapshot_every"] or (a["L"] if "L" in a else max(int(np.max(lens)) if lens is not None else width - a["seed_len"] - 1, 1))
        S = n_steps // every
        local = np.arange(rows)
        ids = np.broadcast_to((100 * np.arange(S)[:, None] + local[None, :])[:, :, None], (S, rows, width)).astype(np.int32)
        cos = (100 * np.arange(S)[:, None] + local[None, :] + 0.5).astype(np.float32) if a["want_cos"] else None
        return ids, cos
    return method


METHOD_NAMES = ["generate_rows", "generate_rows_from", "generate_rows_len", "generate_rows_hp", "generate_rows_draw",
                "generate_rows_tied", "generate_rows_vs"]
for _n in METHOD_NAMES:
    setattr(FakeMember, _n, _recorder(_n))


def make_group(n_members=3):
    grp = EngineGroup.__new__(EngineGroup)
    grp.engines = [FakeMember() for _ in range(n_members)]
    grp.min_images = 2
    grp._pool = None
    grp._full_embeds = grp._encoded = grp._resident = None
    grp.set_image_embeds(EMBEDS)
    return grp


# case -> (method, the arguments it is called with, whole-call snapshot interval, image hand-out mode, tied?)
L_FROM = T - SEED_LEN - 1
CASES = {
    "rows": ("generate_rows", dict(init_ids=INIT[0], L=L_FROM, hyper=HYPERS[0], n_mask=N_MASK), L_FROM, "rows", False),
    "from": ("generate_rows_from", dict(init_rows=INIT, L=L_FROM, hyper=HYPERS[0], n_mask=N_MASK), L_FROM, "rows", False),
    "len": ("generate_rows_len", dict(init_rows=INIT, lens=LENS, hyper=HYPERS[0], n_mask=N_MASK), 6, "rows", False),
    "hp": ("generate_rows_hp", dict(init_rows=INIT, lens=LENS, hypers=HYPERS, n_mask=N_MASK), 6, "rows", False),
    "hp_no_lens": ("generate_rows_hp", dict(init_rows=INIT, lens=None, hypers=HYPERS, n_mask=N_MASK), L_FROM, "rows", False),
    "draw": ("generate_rows_draw", dict(init_rows=INIT, lens=LENS, hypers=HYPERS, draws=DRAWS, n_mask=N_MASK), 6, "rows", False),
    "tied": ("generate_rows_tied", dict(init_rows=INIT, lens=LENS, hypers=HYPERS, draws=DRAWS, groups=GROUPS), 6, "unique", True),
    "vs_tied": ("generate_rows_vs", dict(init_rows=INIT, lens=LENS, hypers=HYPERS, draws=DRAWS, groups=GROUPS, rivals=RIVALS,
                                         deltas=DELTAS), 6, "whole", True),
    "vs": ("generate_rows_vs", dict(init_rows=INIT, lens=LENS, hypers=HYPERS, draws=None, groups=None, rivals=RIVALS, deltas=DELTAS,
                                    n_mask=N_MASK), 6, "whole", False),
}


def run_case(case, n_members=3, **extra):
    method, kw, every, mode, tied = CASES[case]
    grp = make_group(n_members)
    out = getattr(grp, method)(seed_len=SEED_LEN, top_k=TOP_K, positions=POS, image_of_row=IMAGE_OF_ROW, **kw, **extra)
    return grp, out


def member_calls(grp, method):
    """per member that ran: (global rows, the arguments of its one generate call, the embeds it held at that call)"""
    res = []
    for m in grp.engines:
        gen = [(i, a) for i, (n, a) in enumerate(m.calls) if n != "set_image_embeds"]
        if not gen:
            continue
        assert len(gen) == 1 and gen[0][1] is not None
        i, a = gen[0]
        assert m.calls[i - 1][0] == "set_image_embeds" and m.calls[i][0] == method   # the same Engine method, on fresh embeds
        res.append((np.asarray(a["positions"])[0].astype(np.int64), a, m.calls[i - 1][1]["embeds"]))
    return res


@pytest.mark.parametrize("case", list(CASES))
def test_split(case):
    method, kw, every, mode, tied = CASES[case]
    grp, (ids, cos) = run_case(case)
    calls = member_calls(grp, method)
    assert len(calls) >= 2   # R // min_images >= 2: the call is split
    # the parts are disjoint and complete
    assert sorted(np.concatenate([rows for rows, _, _ in calls]).tolist()) == list(range(R))
    for rows, a, emb in calls:
        n = len(rows)
        assert list(rows) == sorted(rows)
        if tied:   # a group is never cut: the rows of the part's groups are all here
            assert set(np.nonzero(np.isin(GROUPS, GROUPS[rows]))[0].tolist()) == set(rows.tolist())
        # exactly its rows' slices of every per-row argument, the arguments shared by all rows as they came
        np.testing.assert_array_equal(np.asarray(a["positions"]), POS[:, rows])
        if method == "generate_rows":
            np.testing.assert_array_equal(np.asarray(a["init_ids"]), INIT[0])
        else:
            np.testing.assert_array_equal(np.asarray(a["init_rows"]), INIT[rows])
        if "lens" in kw:
            if kw["lens"] is None:
                assert a["lens"] is None
            else:
                np.testing.assert_array_equal(np.asarray(a["lens"]), LENS[rows])
        if "hyper" in kw:
            assert a["hyper"] is HYPERS[0]
        if "hypers" in kw:
            assert [h.temperature for h in a["hypers"]] == [HYPERS[r].temperature for r in rows]
        if "draws" in kw:
            assert a["draws"] is None if kw["draws"] is None else [d.seed for d in a["draws"]] == [DRAWS[r].seed for r in rows]
        if "rivals" in kw:
            np.testing.assert_array_equal(np.asarray(a["rivals"]), RIVALS[rows])
            np.testing.assert_array_equal(np.asarray(a["deltas"]), DELTAS[rows])
        if "n_mask" in kw:
            assert list(a["n_mask"]) == N_MASK
        assert a["seed_len"] == SEED_LEN and a["top_k"] == TOP_K
        # group ids: renumbered into [0, rows of the part), the same partition
        if "groups" in kw and kw["groups"] is not None:
            g = np.asarray(a["groups"])
            assert g.shape == (n,) and g.min() >= 0 and g.max() < n
            assert [[g[i] == g[j] for j in range(n)] for i in range(n)] == [[GROUPS[r] == GROUPS[q] for q in rows] for r in rows]
        elif "groups" in a:
            assert a["groups"] is None
        # the images: what the member holds, indexed by what it was told, is each row's own image
        ior = np.arange(n) if a["image_of_row"] is None else np.asarray(a["image_of_row"])
        assert ior.shape == (n,)
        np.testing.assert_array_equal(emb[ior], EMBEDS[IMAGE_OF_ROW[rows]])
        assert {"rows": a["image_of_row"] is None and len(emb) == n,
                "unique": a["image_of_row"] is not None and len(emb) == len(set(IMAGE_OF_ROW[rows].tolist())),
                "whole": a["image_of_row"] is not None and len(emb) == N_IMG}[mode]
        # the snapshot interval is the whole call's for every member (the longest length sits in one part only)
        assert (a["snapshot_every"] or a.get("L")) == every
        # the results: each member-local row at its global index
        S = N_STEPS // every
        assert ids.shape == (S, R, T) and cos.shape == (S, R)
        for s in range(S):
            np.testing.assert_array_equal(ids[s, rows], np.repeat((100 * s + np.arange(n))[:, None], T, axis=1))
            np.testing.assert_array_equal(cos[s, rows], 100 * s + np.arange(n) + 0.5)


@pytest.mark.parametrize("case", [c for c in CASES if "want_cos" in inspect.signature(getattr(EngineGroup, CASES[c][0])).parameters])
def test_want_cos_false_returns_no_cosines(case):
    grp, (ids, cos) = run_case(case, want_cos=False)
    assert cos is None and ids.shape[1:] == (R, T)
    assert all(a["want_cos"] is False for _, a, _ in member_calls(grp, CASES[case][0]))


def test_the_first_two_methods_have_no_want_cos():
    for method in ("generate_rows", "generate_rows_from"):
        assert "want_cos" not in inspect.signature(getattr(EngineGroup, method)).parameters


def test_one_member_gets_the_whole_call():
    grp, (ids, cos) = run_case("tied", n_members=1)
    (rows, a, emb), = member_calls(grp, "generate_rows_tied")
    assert rows.tolist() == list(range(R)) and ids.shape == (N_STEPS // 6, R, T)


@pytest.mark.parametrize("case,upper", [("tied", dict(groups=None)), ("vs_tied", dict(rivals=None)), ("vs_tied", dict(rivals=None, groups=None))])
def test_the_upper_methods_fall_through_to_the_lower_one(case, upper):
    method, kw, every, mode, tied = CASES[case]
    grp = make_group()
    getattr(grp, method)(seed_len=SEED_LEN, top_k=TOP_K, positions=POS, image_of_row=IMAGE_OF_ROW, **{**kw, **upper})
    lower = "generate_rows_tied" if upper.get("groups", GROUPS) is not None else "generate_rows_draw"
    assert {n for m in grp.engines for n, _ in m.calls if n != "set_image_embeds"} == {lower}


def test_refusals_of_the_group_keep_their_texts():
    grp = make_group()
    with pytest.raises(native.NativeError, match=r"EngineGroup\.generate_rows_hp: image_of_row outside the resident image batch"):
        grp.generate_rows_hp(INIT, LENS, SEED_LEN, TOP_K, POS, HYPERS, image_of_row=[0, 1, 2, 3, 0, 1, 2])
    with pytest.raises(native.NativeError, match=r"EngineGroup\.generate_rows_tied: a group id outside \[0, R\)"):
        grp.generate_rows_tied(INIT, LENS, SEED_LEN, TOP_K, POS, HYPERS, DRAWS, [0, 0, 1, 1, 1, 7, 7], image_of_row=IMAGE_OF_ROW)
    with pytest.raises(native.NativeError, match=r"EngineGroup\.generate_rows_vs: groups must hold R ids in \[0, R\)"):
        grp.generate_rows_vs(INIT, LENS, SEED_LEN, TOP_K, POS, HYPERS, DRAWS, [0, 0, 1], RIVALS, DELTAS, image_of_row=IMAGE_OF_ROW)
    with pytest.raises(ValueError, match=r"generate_rows_draw: draws has 2 entries for 7 rows"):
        grp.generate_rows_draw(INIT, LENS, SEED_LEN, TOP_K, POS, HYPERS, DRAWS[:2])
    blank = make_group()
    blank._full_embeds = None
    with pytest.raises(native.NativeError, match=r"EngineGroup\.generate_rows_from: encode_images / set_image_embeds first"):
        blank.generate_rows_from(INIT, L_FROM, SEED_LEN, TOP_K, POS, HYPERS[0])
