"""Per-row visiting orders (czc_generate_rows), host side: the schedules of S samples are drawn exactly as the serial sample
loop draws them, and the C ABI declares the entry point."""
import fnmatch
import os
import random
import re

import numpy as np
import pytest

from conzic_amd import harness, native
from conzic_amd.harness import order_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _serial_draw(order, max_len, max_iters):
    """The statements of runtime.run_generation between the image encode and the engine call, for one sample."""
    order_list = random_positions = None
    if order == "shuffle":
        order_list = list(range(max_len))
        random.shuffle(order_list)
    elif order == "random":
        random_positions = [int(np.random.randint(0, max_len)) for _ in range(max_iters)]
    iters = max_iters if order != "random" else max_iters // max_len
    if order == "random":
        positions, n_mask, every = [int(p) for p in random_positions], [1] * len(random_positions), 1
    else:
        positions, n_mask, every = order_positions(order, max_len, iters, order_list=order_list)
    return positions, n_mask, every, order_list


@pytest.mark.parametrize("order,max_iters", [("shuffle", 3), ("random", 30), ("sequential", 2), ("span", 2)])
def test_sample_schedules_replays_the_serial_loop(order, max_iters):
    L, S = 10, 5
    random.seed(42)
    np.random.seed(42)
    serial = [_serial_draw(order, L, max_iters) for _ in range(S)]
    py_state, np_state = random.getstate(), np.random.get_state()
    random.seed(42)
    np.random.seed(42)
    positions, n_mask, every, order_lists = harness.sample_schedules(order, L, max_iters, S)
    assert positions.dtype == np.int32 and positions.flags.c_contiguous
    assert positions.shape == (len(serial[0][0]), S)
    for s in range(S):
        assert positions[:, s].tolist() == serial[s][0]
        assert n_mask == serial[s][1] and every == serial[s][2]
        assert (order_lists[s] if order_lists is not None else None) == serial[s][3]
    assert random.getstate() == py_state
    got = np.random.get_state()
    assert got[0] == np_state[0] and (got[1] == np_state[1]).all() and got[2:] == np_state[2:]
    if order == "shuffle":
        assert len({tuple(o) for o in order_lists}) > 1  # the samples do differ: the case the rows call exists for


def test_header_declares_and_exports_map_lists_generate_rows():
    with open(native.HEADER_PATH) as f:
        header = f.read()
    assert re.search(r"\bint\s+czc_generate_rows\s*\(\s*czc_engine\s*\*", header)
    assert "CZC_MAX_ROWS" in header
    gen = header[header.index("BEGIN GENERATED"):header.index("END GENERATED")]
    assert "czc_generate_rows" not in gen
    with open(os.path.join(ROOT, "conzic_amd", "csrc", "exports.map")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    globs = re.search(r"global:\s*([^;]+);", text).group(1).split()
    assert any(fnmatch.fnmatchcase("czc_generate_rows", g) for g in globs)
    assert "czc_generate_rows" in native.SIGNATURES
    assert len(native.SIGNATURES["czc_generate_rows"][1]) == 15
