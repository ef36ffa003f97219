"""Host side of mixed caption lengths (conzic_amd/lengths.py, the czc_generate_rows_len binding): no GPU."""
import random
import re

import numpy as np
import pytest

from conzic_amd import lengths, native, synth
from conzic_amd.engine import Engine, EngineGroup
from conzic_amd.text import tokenizers_from_vocab

IDLE = native.POS_IDLE
PROMPT = "Image of a"


@pytest.fixture(scope="module")
def tok():
    return tokenizers_from_vocab(synth.make_vocab_tiny())[0]


@pytest.mark.parametrize("order", ["sequential", "shuffle"])
def test_length_schedules_visit_every_position_once_per_sweep(order):
    lens, sweeps = [3, 6, 4, 6, 1, 5], 3
    pos, n_mask, every = lengths.length_schedules(lens, order, sweeps, rng=random.Random(4))
    assert pos.dtype == np.int32 and pos.shape == (sweeps * 6, 6) and every == 6 and n_mask == [1] * (sweeps * 6)
    for s in range(sweeps):
        sw = pos[s * every:(s + 1) * every]
        np.testing.assert_array_equal(sw, pos[:every])            # one order per row for the whole call
        for r, n in enumerate(lens):
            assert sorted(sw[:n, r].tolist()) == list(range(n))  # each of its positions once, in the sweep's first L_r steps
            assert (sw[n:, r] == IDLE).all()                      # idle for the rest: snapshot s is "after sweep s" for every row
            assert (sw[:n, r] == n - 1).sum() == 1                # the one step that carries the row's '.' rule (position L_r - 1)
            if order == "sequential":
                assert sw[:n, r].tolist() == list(range(n))


def test_shuffle_orders_differ_per_row_and_reproduce_from_the_rng():
    lens = [6, 6, 6, 6]
    a, _, _ = lengths.length_schedules(lens, "shuffle", 1, rng=random.Random(9))
    b, _, _ = lengths.length_schedules(lens, "shuffle", 1, rng=random.Random(9))
    np.testing.assert_array_equal(a, b)
    assert len({tuple(a[:, r].tolist()) for r in range(4)}) > 1
    # one draw per row, in row order, each a shuffle of range(L_r): what a serial loop over the rows draws
    rng = random.Random(9)
    for r in range(4):
        o = list(range(6))
        rng.shuffle(o)
        assert a[:, r].tolist() == o
    random.seed(3)                                                # rng = None: the process-global stream
    c, _, _ = lengths.length_schedules([4, 2], "shuffle", 1)
    random.seed(3)
    o0, o1 = list(range(4)), list(range(2))
    random.shuffle(o0)
    random.shuffle(o1)
    assert c[:, 0].tolist() == o0 and c[:2, 1].tolist() == o1


def test_length_rows_pad_with_zero_behind_sep(tok):
    lens = [2, 5, 1, 7]
    rows = lengths.length_rows(tok, PROMPT, lens)
    seed_len = len(PROMPT.split()) + 1
    assert rows.dtype == np.int32 and rows.shape == (4, seed_len + 7 + 1)
    for r, n in enumerate(lens):
        t_r = seed_len + n + 1
        assert rows[r, :t_r].tolist() == tok.encode(PROMPT + tok.mask_token * n)   # the reference's start row at that length
        assert rows[r, t_r - 1] == tok.sep_token_id
        assert (rows[r, seed_len:seed_len + n] == tok.mask_token_id).all()
        assert (rows[r, t_r:] == 0).all()
    trimmed = lengths.trim_rows(rows, lens, seed_len)
    assert [t.size for t in trimmed] == [seed_len + n + 1 for n in lens]
    assert lengths.decode_rows(tok, rows, lens, seed_len) == [tok.decode(tok.encode(PROMPT + tok.mask_token * n), skip_special_tokens=True)
                                                               for n in lens]


def test_infill_grouping_of_a_call_is_one_group(tok):
    from conzic_amd import infill
    caps = ["the _ picture of _ _", "_ photos _", "_ picture _ the _ photo", "_"]
    parsed = [infill.parse_template(tok, PROMPT, c) for c in caps]
    assert len({len(p[0]) for p in parsed}) == 3                 # three token lengths ...
    groups = infill.group_for_call(parsed)
    assert list(groups.items()) == [(max(len(p[0]) for p in parsed), [0, 1, 2, 3])]   # ... one call, keyed by its row stride
    assert infill.group_for_call([]) == {}
    other = infill.parse_template(tok, "Image of", "a _")        # another prompt: another seed_len, not one call
    with pytest.raises(ValueError):
        infill.group_for_call(parsed + [other])
    # the order run_infill logs and returns in is still by token length, first appearance first
    assert list(infill.group_by_length(parsed).values()) == [[0, 2], [1], [3]]


def test_wrappers_reject_bad_shapes(tok):
    with pytest.raises(ValueError):
        lengths.length_schedules([], "shuffle", 1)
    with pytest.raises(ValueError):
        lengths.length_schedules([3, 0], "shuffle", 1)
    with pytest.raises(ValueError):
        lengths.length_schedules([3, 4], "random", 1)
    with pytest.raises(ValueError):
        lengths.length_rows(tok, PROMPT, [])
    with pytest.raises(ValueError):
        lengths.trim_rows(np.zeros((2, 6), np.int32), [3, 4], 4)
    eng = Engine.__new__(Engine)   # the shape checks come before the library is touched
    hp = Engine.hyper(0.02, 2.0, 0.1)
    rows, pos = np.zeros((3, 9), np.int32), np.zeros((4, 3), np.int32)
    for kw in (dict(init_rows=rows[:2]), dict(lens=[2, 3]), dict(positions=pos[:, 0]), dict(image_of_row=[0, 1]), dict(n_mask=[1, 1])):
        a = dict(init_rows=rows, lens=[2, 3, 4], positions=pos, image_of_row=None, n_mask=None)
        a.update(kw)
        with pytest.raises(ValueError):
            eng.generate_rows_len(a["init_rows"], a["lens"], 4, 8, a["positions"], hp, image_of_row=a["image_of_row"], n_mask=a["n_mask"])
    from conzic_amd import runtime
    for bad in (dict(lens=[]), dict(lens=[4, 0]), dict(generate_order="random"), dict(generate_order="span")):
        a = dict(lens=[4, 6], generate_order="shuffle")
        a.update(bad)
        with pytest.raises(ValueError):   # before any engine is built
            runtime.caption_lengths(a["lens"], 1, "caption", ["img0"], None, None, tok, None, None, None, prompt=PROMPT,
                                    generate_order=a["generate_order"])
    grp = EngineGroup.__new__(EngineGroup)
    with pytest.raises(ValueError):
        grp.generate_rows_len(rows, [2, 3], 4, 8, pos, hp)


def test_library_binding_of_generate_rows_len():
    lib = native.load()
    assert lib.czc_version() >= 101
    fn = lib.czc_generate_rows_len
    res, args = native.SIGNATURES["czc_generate_rows_len"]
    assert fn.restype is res and list(fn.argtypes) == args
    hdr = open(native.HEADER_PATH).read()
    decl = re.search(r"int czc_generate_rows_len\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(args) and "len_of_row_host" in decl
    assert fn(None, 1, 1, 0, None, None, None, 1, 0, None, None, 1, None, None, None) == native.ERR_ARG   # no engine: refused, no GPU touched
