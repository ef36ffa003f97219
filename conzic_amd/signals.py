"""One image under several control signals in one batch on czc_generate_rows_hp (include/conzic_hip.h): host-side parsing and
row expansion.

The reference runs one control signal per process (--run_type caption | controllable, --control_type sentiment | pos,
--sentiment_type positive | negative).  A row of a czc_generate_rows_hp call has its own czc_hyper, so a plain caption, a positive
one, a negative one and a POS-templated one of the same image are four rows of one call.  Everything here is NumPy on the host."""
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from . import lengths, native

SIGNALS = ("caption", "positive", "negative", "pos")


def parse_signals(text) -> List[str]:
    """`caption,positive,negative,pos` (or a sequence of such names) -> the list of signals, in the order given.  An empty list,
    an unknown name and a name given twice raise ValueError."""
    names = [s.strip().lower() for s in (text.split(",") if isinstance(text, str) else list(text))]
    names = [s for s in names if s]
    if not names:
        raise ValueError(f"no control signal given; expected a comma-separated list of {'|'.join(SIGNALS)}")
    for s in names:
        if s not in SIGNALS:
            raise ValueError(f"unknown control signal {s!r}; expected one of {'|'.join(SIGNALS)}")
    if len(set(names)) != len(names):
        raise ValueError(f"a control signal is given twice in {names!r}")
    return names


def signal_run(signal: str):
    """(run_type, ctl_type, style_type) of the reference run a signal stands for (demo.py:34-46)."""
    if signal not in SIGNALS:
        raise ValueError(f"unknown control signal {signal!r}")
    if signal == "caption":
        return "caption", "sentiment", "positive"
    if signal == "pos":
        return "controllable", "pos", "positive"
    return "controllable", "sentiment", signal


def signal_hyper(signal: str, alpha: float, beta: float, temperature: float, gamma: float) -> native.Hyper:
    """The czc_hyper of a row under `signal`: control 0 (gamma unused) for a caption, 1 with the sign for a sentiment, 2 for POS."""
    from .engine import Engine
    run_type, ctl_type, style = signal_run(signal)
    if run_type == "caption":
        return Engine.hyper(alpha, beta, temperature)
    return Engine.hyper(alpha, beta, temperature, gamma, style == "negative", control="pos" if ctl_type == "pos" else None)


def signal_order(signal: str, generate_order: str, max_iter: int, max_len: int):
    """(visiting order, sweeps) of the *_generation function behind a signal's run (runtime.caption_order): a caption run keeps
    --order, a sentiment run turns everything but `sequential` into `shuffle`, a POS run is sequential."""
    from . import runtime
    run_type, ctl_type, _ = signal_run(signal)
    return runtime.caption_order(run_type, generate_order, ctl_type, max_iter, max_len)


@dataclass
class SignalRows:
    """Columns of a signals call (one per signal, length and sample; a batch of B images repeats every column B times)."""
    signals: List[str]
    lens: List[int]
    samples: int
    col_signal: List[int]        # column -> index into signals
    col_lens: List[int]          # column -> sentence length
    orders: List[str]            # per signal: its visiting order
    positions: np.ndarray        # int32 [sweeps * max(lens), columns], native.POS_IDLE behind a shorter row's positions
    n_mask: List[int]
    every: int                   # steps per sweep = snapshot interval
    sweeps: int
    hypers: List[native.Hyper]   # per column

    def column(self, g: int, l: int, s: int) -> int:
        return (g * len(self.lens) + l) * self.samples + s


def expand(signals: Sequence[str], lens: Sequence[int], samples: int, generate_order: str, max_iter: int, *, alpha: float,
           beta: float, temperature: float, gamma: float, rng=None) -> SignalRows:
    """signals x lengths x samples -> columns, column (g * len(lens) + l) * samples + s = sample s at lens[l] under signals[g].
    Every column gets the visiting order the reference would have drawn for that run and sample: the orders are drawn in the
    order a serial loop over signals, then lengths, then samples draws them (lengths.length_schedules per signal: one shuffle per
    shuffled column from `rng`, None = the process-global `random` stream; sequential columns draw nothing), so the captions of
    the one call are that loop's.  `generate_order` must leave every signal sequential or shuffle."""
    signals = parse_signals(signals)
    lens = [int(n) for n in lens]
    S = int(samples)
    if not lens or min(lens) < 1 or S < 1:
        raise ValueError(f"signals: lengths {lens!r} must be >= 1 and samples = {S} >= 1")
    col_lens_sig = [n for n in lens for _ in range(S)]
    blocks, orders, sweeps_all = [], [], []
    n_mask, every = None, max(lens)
    for sig in signals:
        order, sweeps = signal_order(sig, generate_order, max_iter, max(lens))
        if order not in lengths.ORDERS:
            raise ValueError(f"signals in one call need an order of sequential|shuffle for every signal, got {order!r} for {sig!r}")
        pos, n_mask, every = lengths.length_schedules(col_lens_sig, order, sweeps, rng=rng)
        blocks.append(pos)
        orders.append(order)
        sweeps_all.append(int(sweeps))
    if len(set(sweeps_all)) != 1:
        raise ValueError(f"signals in one call need one number of sweeps, got {sweeps_all!r}")
    positions = np.ascontiguousarray(np.concatenate(blocks, axis=1))
    col_signal = [g for g in range(len(signals)) for _ in col_lens_sig]
    hypers = [signal_hyper(signals[g], alpha, beta, temperature, gamma) for g in col_signal]
    return SignalRows(signals, lens, S, col_signal, col_lens_sig * len(signals), orders, positions, list(n_mask), int(every),
                      sweeps_all[0], hypers)


def batch_rows(rows: SignalRows, tokenizer, prompt: str, batch_size: int):
    """The arguments of Engine.generate_rows_hp for a batch of `batch_size` images: row c * batch_size + b = column c of image b.
    Returns (init_rows [R, T], row_lens [R], positions [n_steps, R], hypers [R], image_of_row [R])."""
    B = int(batch_size)
    col_rows = lengths.length_rows(tokenizer, prompt, rows.col_lens)
    init_rows = np.ascontiguousarray(np.repeat(col_rows, B, axis=0))
    row_lens = np.repeat(np.asarray(rows.col_lens, dtype=np.int32), B)
    positions = np.ascontiguousarray(np.repeat(rows.positions, B, axis=1))
    hypers = [h for h in rows.hypers for _ in range(B)]
    image_of_row = np.tile(np.arange(B, dtype=np.int32), len(rows.col_lens))
    return init_rows, row_lens, positions, hypers, image_of_row
