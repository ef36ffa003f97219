"""Host side of control signals in one batch (conzic_amd/signals.py, the czc_generate_rows_hp binding): no GPU."""
import random

import numpy as np
import pytest

from conzic_amd import lengths, native, runtime, signals, synth
from conzic_amd.engine import Engine, hyper_array
from conzic_amd.text import tokenizers_from_vocab

IDLE = native.POS_IDLE
PROMPT = "Image of a"
HP = dict(alpha=0.02, beta=2.0, temperature=0.1, gamma=5.0)


def test_parse_signals():
    assert signals.parse_signals("caption,positive,negative,pos") == ["caption", "positive", "negative", "pos"]
    assert signals.parse_signals(" Negative , caption ") == ["negative", "caption"]
    assert signals.parse_signals(["pos"]) == ["pos"]
    for bad in ("", " , ", [], "caption,happy", "sentiment", "caption,caption"):
        with pytest.raises(ValueError):
            signals.parse_signals(bad)


def test_signal_run_hyper_and_order():
    assert signals.signal_run("caption") == ("caption", "sentiment", "positive")
    assert signals.signal_run("negative") == ("controllable", "sentiment", "negative")
    assert signals.signal_run("pos") == ("controllable", "pos", "positive")
    with pytest.raises(ValueError):
        signals.signal_run("neutral")
    want = {"caption": (0, 0, 0.0), "positive": (1, 0, 5.0), "negative": (1, 1, 5.0), "pos": (2, 0, 5.0)}
    for sig, (control, negative, gamma) in want.items():
        h = signals.signal_hyper(sig, **HP)
        assert (h.control, h.negative, h.gamma) == (control, negative, gamma)
        assert (h.alpha, h.beta, h.temperature) == tuple(np.float32(v) for v in (0.02, 2.0, 0.1))
    # the order of the *_generation function behind each run (runtime.caption_order)
    assert [signals.signal_order(s, "shuffle", 3, 6) for s in signals.SIGNALS] == \
        [("shuffle", 3), ("shuffle", 3), ("shuffle", 3), ("sequential", 3)]
    assert [signals.signal_order(s, "sequential", 3, 6)[0] for s in signals.SIGNALS] == ["sequential"] * 4


def test_expand_rows():
    sigs, lens, S, B = ["caption", "positive", "negative", "pos"], [4, 6], 2, 3
    rows = signals.expand(sigs, lens, S, "shuffle", 2, rng=random.Random(1), **HP)
    n_col = len(sigs) * len(lens) * S
    assert len(rows.col_signal) == len(rows.col_lens) == len(rows.hypers) == n_col
    assert rows.positions.shape == (2 * 6, n_col) and rows.every == 6 and rows.sweeps == 2 and rows.n_mask == [1] * 12
    assert rows.col_signal == [g for g in range(4) for _ in range(4)]
    assert rows.col_lens == [4, 4, 6, 6] * 4
    assert rows.orders == ["shuffle", "shuffle", "shuffle", "sequential"]
    for g, sig in enumerate(sigs):
        for l, n in enumerate(lens):
            for s in range(S):
                c = rows.column(g, l, s)
                assert rows.col_signal[c] == g and rows.col_lens[c] == n
                assert bytes(rows.hypers[c]) == bytes(signals.signal_hyper(sig, **HP))
                col = rows.positions[:6, c]
                assert sorted(col[:n].tolist()) == list(range(n)) and (col[n:] == IDLE).all()
                if sig == "pos":
                    assert col[:n].tolist() == list(range(n))
    assert [h.control for h in rows.hypers] == [0] * 4 + [1] * 8 + [2] * 4
    assert [h.negative for h in rows.hypers] == [0] * 8 + [1] * 4 + [0] * 4
    tok = tokenizers_from_vocab(synth.make_vocab_tiny())[0]
    init, row_lens, pos, hps, ior = signals.batch_rows(rows, tok, PROMPT, B)
    R = n_col * B
    assert init.shape == (R, 4 + 6 + 1) and row_lens.tolist() == [n for n in rows.col_lens for _ in range(B)]
    assert pos.shape == (12, R) and ior.tolist() == list(range(B)) * n_col and len(hps) == R
    for c in range(n_col):
        for b in range(B):
            r = c * B + b
            np.testing.assert_array_equal(pos[:, r], rows.positions[:, c])
            np.testing.assert_array_equal(init[r], lengths.length_rows(tok, PROMPT, rows.col_lens)[c])
            assert bytes(hps[r]) == bytes(rows.hypers[c])
    arr = hyper_array(hps)
    assert len(arr) == R and [a.control for a in arr] == [h.control for h in hps]
    with pytest.raises(ValueError):
        signals.expand(sigs, [], S, "shuffle", 2, **HP)
    with pytest.raises(ValueError):
        signals.expand(sigs, lens, 0, "shuffle", 2, **HP)
    with pytest.raises(ValueError):
        signals.expand(["caption"], lens, 1, "random", 2, **HP)   # a caption run's random order has no per-row schedule


@pytest.mark.parametrize("order", ["shuffle", "sequential"])
def test_orders_are_the_serial_loops(order):
    """Python's `random` and numpy seeded: the expanded columns carry the orders a serial loop over signals, lengths and samples
    draws with the existing runtime helpers (runtime.caption_order for the run's order, lengths.length_schedules for one run's
    draw: what run_generation_lengths calls), and the global RNG state afterwards is that loop's."""
    sigs, lens, S, iters = ["caption", "positive", "negative", "pos"], [3, 5, 6], 2, 2
    random.seed(7)
    np.random.seed(7)
    serial = []
    for sig in sigs:
        run_type, ctl_type, _ = signals.signal_run(sig)
        o, sweeps = runtime.caption_order(run_type, order, ctl_type, iters, max(lens))
        for n in lens:
            for _ in range(S):
                p, _, _ = lengths.length_schedules([n], o, sweeps)
                serial.append(p[:n, 0].tolist())
    st_py, st_np = random.getstate(), np.random.get_state()
    random.seed(7)
    np.random.seed(7)
    rows = signals.expand(sigs, lens, S, order, iters, **HP)
    assert random.getstate() == st_py
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), st_np))
    got = [rows.positions[:n, c].tolist() for c, n in enumerate(rows.col_lens)]
    assert got == serial
    if order == "shuffle":
        assert len({tuple(o) for o, n in zip(got, rows.col_lens) if n == 6}) > 1


def test_library_binding_of_generate_rows_hp():
    lib = native.load()
    assert lib.czc_version() >= 102
    fn = lib.czc_generate_rows_hp
    assert len(fn.argtypes) == len(lib.czc_generate_rows_len.argtypes)
    hp = [Engine.hyper(0.02, 2.0, 0.1)] * 2
    # a NULL engine is refused before anything is read
    assert fn(None, 2, 8, 4, None, None, None, 8, 0, None, None, 1, hyper_array(hp), None, None) == native.ERR_ARG
    with pytest.raises(TypeError):
        hyper_array([object()])
