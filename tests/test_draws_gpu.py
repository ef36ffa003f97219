"""-m gpu: --sample_tau of the CLIs (runtime.run_generation_samples / _lengths / _signals / run_infill on
czc_generate_rows_draw).  Under --order sequential the argmax rule returns the same caption for every sample of an image; with a
tau every (image, sample) draws under its own seed, and the one batched call returns what the sample loop returns."""
import logging

import pytest

pytestmark = pytest.mark.gpu
BASE = ["--synthetic", "--tiny", "--run_type", "caption", "--order", "sequential", "--samples_num", "4", "--sentence_len", "5",
        "--num_iterations", "2", "--candidate_k", "50"]


def _run(argv, caplog):
    from conzic_amd import demo_cli, runtime
    caplog.clear()
    try:
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            demo_cli.main(argv)
    finally:
        runtime.evict()
    return [r.getMessage() for r in caplog.records]


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_sampled_samples_differ_and_the_batched_call_is_the_sample_loop(prec, monkeypatch, caplog):
    monkeypatch.setenv("CZC_PRECISION", prec)
    monkeypatch.delenv("CZC_MEMO_ROWS", raising=False)
    finals = {}
    for tag, extra in (("argmax", []), ("loop", ["--sample_tau", "0.5"]), ("batched", ["--sample_tau", "0.5", "--batch_samples"])):
        msgs = _run(BASE + extra, caplog)
        finals[tag] = [m for m in msgs if m.startswith("final caption: ")]
        assert len(finals[tag]) == 4
        div = [m for m in msgs if m.startswith("diversity of 4 samples of img0")]
        assert len(div) == 1
        said = [m for m in msgs if m.startswith("Order:sequential sample_tau 0.5 seeds [0x")]
        assert len(said) == (0 if tag == "argmax" else 4) and len(set(said)) == len(said)
        if tag == "batched":
            assert sorted(said) == sorted(loop_said)
        loop_said = said
    print(finals)
    assert len(set(finals["argmax"])) == 1          # the gap: four equal captions
    assert len(set(finals["loop"])) > 1             # closed: the samples differ ...
    assert finals["batched"] == finals["loop"]      # ... reproducibly, whichever way they are batched


def test_sample_tau_with_lengths_signals_and_infill(monkeypatch, caplog):
    from conzic_amd import runtime
    monkeypatch.setenv("CZC_PRECISION", "bf16")
    got = []
    real = runtime.caption_signals
    monkeypatch.setattr(runtime, "caption_signals", lambda *a, **k: got.append(real(*a, **k)) or got[-1])
    msgs = _run(["--synthetic", "--tiny", "--order", "sequential", "--samples_num", "2", "--num_iterations", "2", "--candidate_k", "50",
                 "--batch_size", "2", "--control_scores", "table", "--signals", "caption,positive", "--sentence_lens", "4,6",
                 "--batch_samples", "--sample_tau", "0.5"], caplog)
    (outs,) = got
    assert len(outs) == 2 and all(len(per_len) == 2 for per_len in outs)           # signals x lengths
    for per_len in outs:
        for per_sample in per_len:
            assert len(per_sample) == 2                                            # samples
            for texts, scores in per_sample:
                assert len(texts) == 3 and len(scores) == 3 and all(len(t) == 2 for t in texts)   # two sweeps + best, two images
    said = [m for m in msgs if " sample_tau 0.5 seeds [0x" in m]
    assert len(said) == 8 and len(set(said)) == 8                                  # a seed pair per signal, length and sample
    assert sum(m.startswith("final caption: ") for m in msgs) == 16
    # the sample loop over the same lengths, and an infill call
    msgs = _run(["--synthetic", "--tiny", "--run_type", "caption", "--order", "shuffle", "--samples_num", "2", "--num_iterations", "2",
                 "--candidate_k", "50", "--sentence_lens", "4,6", "--sample_tau", "0.5"], caplog)
    assert sum(m.startswith("final caption: ") for m in msgs) == 4
    assert sum(m.startswith("Order_list:") and " sample_tau 0.5 seeds [0x" in m for m in msgs) == 4
    msgs = _run(["--synthetic", "--tiny", "--run_type", "infill", "--order", "sequential", "--num_iterations", "2", "--candidate_k", "50",
                 "--caption", "the _ picture of _ _", "--caption", "_ photos _", "--sample_tau", "0.5"], caplog)
    assert sum(m.startswith("final caption: ") for m in msgs) == 2
    assert sum(m.startswith("Order:sequential sample_tau 0.5 seeds [0x") for m in msgs) == 2
