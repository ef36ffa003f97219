"""`--fluency` / `--pick_lambda` of conzic_amd.demo_cli on the tiny synthetic towers: the logged pseudo-log-likelihoods are those of
an Engine.fluency_rows call on the final ids, and the flag changes nothing else the run logs or returns."""
import logging
import re

import numpy as np
import pytest

from conzic_amd import fluency

pytestmark = pytest.mark.gpu

BASE = ["--synthetic", "--tiny", "--samples_num", "3", "--sentence_len", "5", "--candidate_k", "12", "--num_iterations", "2",
        "--batch_size", "2", "--order", "shuffle"]
MODES = {
    "serial": ["--run_type", "caption"],
    "batch_samples": ["--run_type", "caption", "--batch_samples"],
    "sample_tau": ["--run_type", "caption", "--sample_tau", "0.5"],
    "controllable": ["--run_type", "controllable", "--control_scores", "table", "--batch_samples"],
}
KEPT = ("Order_list", "iter ", "final caption", "best caption")   # what the run logs without the flag (timings aside)


def _run(argv, caplog):
    from conzic_amd import demo_cli
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="ConZIC"):
        finals = demo_cli.main(argv)
    return finals, [r.getMessage() for r in caplog.records]


@pytest.mark.parametrize("mode", list(MODES))
def test_fluency_flag_logs_the_engine_call_and_changes_nothing_else(mode, caplog, monkeypatch):
    from conzic_amd import runtime
    calls = []
    real = runtime.caption_fluency

    def spy(eng, ids, seed_len, lens, *a, **kw):
        recs = real(eng, ids, seed_len, lens, *a, **kw)
        again = eng.fluency_rows(np.ascontiguousarray(ids, dtype=np.int32), seed_len, lens=lens)   # the same call: the same bits
        calls.append((np.array(ids), fluency.summarize(again["logp"], again["rank"], lens), recs))
        return recs
    try:
        plain_finals, plain = _run(BASE + MODES[mode], caplog)
        runtime.evict()
        monkeypatch.setattr(runtime, "caption_fluency", spy)
        flu_finals, flu = _run(BASE + MODES[mode] + ["--pick_lambda", "0"], caplog)
    finally:
        runtime.evict()
    assert flu_finals == plain_finals
    for kind in KEPT:
        assert [m for m in flu if m.startswith(kind)] == [m for m in plain if m.startswith(kind)], kind
    assert not any("fluency: PLL" in m or "picked caption" in m for m in plain)
    # one line per (sample, image), each with the PLL of the direct call on the final ids
    lines = [m for m in flu if "fluency: PLL" in m]
    want = [f"fluency: PLL {d['pll']:.4f}, mean log p {d['mean_logp']:.4f}," for _, direct, _ in calls for d in direct]
    assert len(lines) == 3 * 2 == len(want)
    for line, w in zip(lines, want):
        assert w in line, (line, w)
    for ids, direct, recs in calls:
        assert ids.ndim == 2 and len(direct) == len(recs) == len(ids)
    # --pick_lambda 0: per image, the sample with the largest final cosine (the first on ties)
    recs = [r for _, _, rs in calls for r in rs]
    picked = [m for m in flu if "picked caption" in m]
    assert len(picked) == 2
    for b, line in enumerate(picked):
        mine = sorted((r for r in recs if r["image"] == b), key=lambda r: r["sample"])
        assert [r["sample"] for r in mine] == [0, 1, 2]
        best = int(np.argmax([r["cos"] for r in mine]))
        assert int(re.search(r"picked caption \(sample (\d+),", line).group(1)) == best, (line, [r["cos"] for r in mine])
        assert line.startswith(f"The {b + 1}-th image: img{b}, picked caption")
