"""Host side of infilling (conzic_amd/infill.py, the czc_generate_rows_from binding): no GPU."""
import random
import re

import numpy as np
import pytest

from conzic_amd import infill, native, synth
from conzic_amd.text import tokenizers_from_vocab

IDLE = native.POS_IDLE


@pytest.fixture(scope="module")
def tok():
    return tokenizers_from_vocab(synth.make_vocab_tiny())[0]


def test_parse_template_with_and_without_a_prompt(tok):
    ids, blanks, L, seed_len = infill.parse_template(tok, "Image of a", "_ picture of _ photos _")
    v = tok.vocab
    assert seed_len == 4 and L == 7 and ids.size == seed_len + L + 1 and ids.dtype == np.int32
    assert ids.tolist() == [v["[CLS]"], v["image"], v["of"], v["a"], v["[MASK]"], v["picture"], v["of"], v["[MASK]"], v["photo"],
                            v["##s"], v["[MASK]"], v["[SEP]"]]
    assert blanks == [0, 3, 6]                                   # every blank is one [MASK]; the two-piece word is kept
    assert all(ids[seed_len + p] == tok.mask_token_id for p in blanks)
    assert ids.tolist() == tok.encode("Image of a" + " [MASK] picture of [MASK] photos [MASK]")
    ids, blanks, L, seed_len = infill.parse_template(tok, "", "the _ photo")
    assert seed_len == 1 and L == 3 and blanks == [1]
    assert ids.tolist() == [v["[CLS]"], v["the"], v["[MASK]"], v["photo"], v["[SEP]"]]
    ids, blanks, L, seed_len = infill.parse_template(tok, "Image of a", "the picture")   # a draft without blanks
    assert blanks == [] and L == 2 and seed_len == 4
    ids, blanks, L, _ = infill.parse_template(tok, "Image of a", "the * photo *", blank="*")
    assert blanks == [1, 3] and L == 4
    # all blanks: the engine's standard init row (utils.get_init_text)
    ids, blanks, L, seed_len = infill.parse_template(tok, "Image of a", "_ _ _ _")
    assert ids.tolist() == tok.encode("Image of a" + tok.mask_token * 4) and blanks == [0, 1, 2, 3]


@pytest.mark.parametrize("order", ["sequential", "shuffle"])
def test_infill_schedules_visit_every_blank_once_per_sweep(order):
    blank_sets = [[0, 2, 5, 6], [1], [], [3, 4, 6], [6, 0]]
    sweeps = 3
    random.seed(5)
    pos, n_mask, every = infill.infill_schedules(blank_sets, order, sweeps)
    assert pos.dtype == np.int32 and pos.shape == (sweeps * 4, 5) and every == 4 and n_mask == [1] * 12
    for s in range(sweeps):
        sw = pos[s * every:(s + 1) * every]
        np.testing.assert_array_equal(sw, pos[:every])           # one order per row for the whole call
        for r, bl in enumerate(blank_sets):
            col = sw[:, r]
            assert sorted(col[col != IDLE].tolist()) == sorted(bl)          # each blank exactly once
            assert (col[len(bl):] == IDLE).all() and (col[:len(bl)] != IDLE).all()   # the rest is idle, at the end of the sweep
            if order == "sequential":
                assert col[:len(bl)].tolist() == sorted(bl)
    random.seed(5)
    again, _, _ = infill.infill_schedules(blank_sets, order, sweeps)
    np.testing.assert_array_equal(pos, again)                    # deterministic under random.seed
    # the global stream moves by one shuffle per row, in row order (sequential: not at all)
    random.seed(5)
    want = []
    for bl in blank_sets:
        lst = list(bl)
        if order == "shuffle":
            random.shuffle(lst)
        want.append(lst if order == "shuffle" else sorted(lst))
    after = random.random()
    random.seed(5)
    infill.infill_schedules(blank_sets, order, sweeps)
    assert random.random() == after
    assert [pos[:len(w), r].tolist() for r, w in enumerate(want)] == want
    # an rng of the caller's leaves the global stream alone
    random.seed(5)
    first = random.random()
    random.seed(5)
    infill.infill_schedules(blank_sets, "shuffle", 1, rng=random.Random(1))
    assert random.random() == first


def test_infill_schedules_edge_cases():
    pos, n_mask, every = infill.infill_schedules([[], []], "sequential", 4)
    assert pos.shape == (0, 2) and n_mask == [] and every == 1
    with pytest.raises(ValueError):
        infill.infill_schedules([[1, 1]], "sequential", 1)
    with pytest.raises(ValueError):
        infill.infill_schedules([[1]], "span", 1)
    assert infill.last_visited(np.array([[0, 1], [2, IDLE], [IDLE, IDLE]])) == 2
    assert infill.last_visited(np.full((2, 2), IDLE)) is None


def test_grouping_by_token_length(tok):
    caps = ["_ picture _", "the _ photo of _", "photos _ _", "_ _ _ _ _", "the picture"]
    parsed = [infill.parse_template(tok, "Image of a", c) for c in caps]
    groups = infill.group_by_length(parsed)
    assert [len(p[0]) for p in parsed] == [8, 10, 9, 10, 7]     # "photos" is two pieces
    assert groups == {8: [0], 10: [1, 3], 9: [2], 7: [4]}
    assert list(groups) == [8, 10, 9, 7]                         # first appearance
    visits = infill.visit_lists(parsed)
    assert visits == [[0, 2], [1, 4], [2, 3], [0, 1, 2, 3, 4], []]
    assert infill.visit_lists(parsed, "all") == [list(range(p[2])) for p in parsed]
    # a group's schedule: its captions' columns, every sweep cut to the group's longest row
    pos_all, _, every_all = infill.infill_schedules(visits, "sequential", 2)
    assert every_all == 5 and pos_all.shape == (10, 5)
    pos, n_mask, every = infill.take_rows(pos_all, 2, groups[10])
    assert every == 5 and pos.shape == (10, 2) and n_mask == [1] * 10
    pos, n_mask, every = infill.take_rows(pos_all, 2, groups[8])
    assert every == 2 and pos[:, 0].tolist() == [0, 2, 0, 2]
    alone, _, _ = infill.infill_schedules([visits[0]], "sequential", 2)
    np.testing.assert_array_equal(pos, alone)                    # what the caption gets in a call of its own
    pos, n_mask, every = infill.take_rows(pos_all, 2, groups[7])
    assert pos.shape == (0, 1) and every == 1


def test_library_binding_of_generate_rows_from():
    lib = native.load()
    fn = lib.czc_generate_rows_from
    res, args = native.SIGNATURES["czc_generate_rows_from"]
    assert fn.restype is res and list(fn.argtypes) == args
    assert args == native.SIGNATURES["czc_generate_rows"][1]     # the declared signature: czc_generate_rows' argument list
    hdr = open(native.HEADER_PATH).read()
    assert re.search(r"#define\s+CZC_POS_IDLE\s+\(-1\)", hdr) and native.POS_IDLE == -1
    decl = re.search(r"int czc_generate_rows_from\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(args)
    assert fn(None, 1, 1, 1, 0, None, None, 1, 0, None, None, 1, None, None, None) == native.ERR_ARG   # no engine: refused, no GPU touched


def test_cli_knows_the_infill_run_type():
    from conzic_amd.demo_cli import get_args
    a = get_args(["--run_type", "infill", "--caption", "a _ dog", "--caption", "_ cat", "--order", "sequential"])
    assert a.run_type == "infill" and a.caption == ["a _ dog", "_ cat"] and a.infill_positions == "blanks"
    assert get_args([]).caption is None and get_args([]).run_type == "controllable"   # default off
    with pytest.raises(SystemExit):
        get_args(["--run_type", "infill"])
