"""-m gpu: block-synchronous sweeps above the C ABI -- runtime.run_generation_blocks, EngineGroup.generate_rows_tied and
--block_width of the CLIs.  Tiny synthetic towers, K = 200 (50 through the CLI), two sweeps."""
import logging
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PROMPT = "Image of a"
K = 200
L = 5


def _models(B):
    from PIL import Image
    from clip.clip import CLIP
    from conzic_amd import synth
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab
    sv = synth.make_vocab_tiny()
    bcfg, ccfg = synth.bert_tiny(len(sv.bert_tokens)), synth.clip_tiny(len(sv.clip_vocab))
    tok, clip_tok = tokenizers_from_vocab(sv)
    clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, 12), clip_tok)
    images = [Image.fromarray(u) for u in synth.make_images_u8(B, ccfg.v_image)]
    return SyntheticLM(bcfg), clip, tok, (images if B > 1 else images[0]), synth.make_token_mask(sv), [f"img{j}" for j in range(B)]


def _msgs(caplog):
    return [r.getMessage() for r in caplog.records]


@pytest.mark.parametrize("order", ["sequential", "shuffle"])
def test_width_one_is_run_generation(order, monkeypatch, caplog):
    from conzic_amd import runtime
    monkeypatch.setenv("CZC_PRECISION", "f32")
    B = 2
    lm, clip, tok, imgs, mask, names = _models(B)
    logger = logging.getLogger("ConZIC")
    try:
        random.seed(5)
        want = runtime.run_generation(order, names, lm, clip, tok, imgs, mask.copy(), PROMPT, logger, L, K, 0.1, 0.02, 2.0, 2, B)
        random.seed(5)
        (got,) = runtime.run_generation_blocks(order, 1, "interleaved", 1, names, lm, clip, tok, imgs, mask.copy(), PROMPT, logger,
                                               L, K, 0.1, 0.02, 2.0, 2, B)
        assert got[0] == want[0] and len(got[0]) == 3
        np.testing.assert_array_equal(np.array(got[1], dtype=np.float32), np.array(want[1], dtype=np.float32))
        for bad in ("span", "random"):
            with pytest.raises(ValueError):
                runtime.run_generation_blocks(bad, 2, "interleaved", 1, names, lm, clip, tok, imgs, mask.copy(), PROMPT, logger, L, K,
                                              0.1, 0.02, 2.0, 2, B)
        with pytest.raises(ValueError):
            runtime.run_generation_blocks(order, 2, "diagonal", 1, names, lm, clip, tok, imgs, mask.copy(), PROMPT, logger, L, K,
                                          0.1, 0.02, 2.0, 2, B)
    finally:
        runtime.evict()


@pytest.mark.parametrize("order", ["sequential", "shuffle"])
def test_batched_samples_at_full_width_are_the_samples_alone(order, monkeypatch, caplog):
    """Width L (given as 0), two images x three samples that draw (sample_tau 0.5, so the samples differ): every sample of the
    one call returns what a tied call of that sample alone returns -- texts equal, merged cosines within 2e-6 (F32)."""
    from conzic_amd import runtime
    monkeypatch.setenv("CZC_PRECISION", "f32")
    B, S = 2, 3
    lm, clip, tok, imgs, mask, names = _models(B)
    logger = logging.getLogger("ConZIC")
    kw = dict(sample_tau=0.5, sample_seed=9)
    try:
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            random.seed(5)
            both = runtime.run_generation_blocks(order, 0, "interleaved", S, names, lm, clip, tok, imgs, mask.copy(), PROMPT, logger,
                                                 L, K, 0.1, 0.02, 2.0, 2, B, **kw)
            random.seed(5)
            alone = [runtime.run_generation_blocks(order, 0, "interleaved", 1, names, lm, clip, tok, imgs, mask.copy(), PROMPT,
                                                   logger, L, K, 0.1, 0.02, 2.0, 2, B, sample0=s, **kw)[0] for s in range(S)]
        assert len(both) == S
        for s in range(S):
            assert both[s][0] == alone[s][0]
            assert len(both[s][0]) == 3 and len(both[s][0][0]) == B          # two sweeps + best, per image
            assert np.abs(np.array(both[s][1], dtype=np.float64) - np.array(alone[s][1], dtype=np.float64)).max() <= 2e-6
            # "best" is chosen by the merged captions' cosines
            for b in range(B):
                vals = [both[s][1][i][b] for i in range(2)]
                sweep = int(np.argmax(vals))
                if max(vals) > 0:       # (gen_utils.py:82-96 starts from score 0 and caption 'None')
                    assert both[s][0][-1][b] == both[s][0][sweep][b] and both[s][1][-1][b] == vals[sweep]
                else:
                    assert both[s][0][-1][b] == 'None' and both[s][1][-1][b] == 0
        assert len({tuple(both[s][0][-2]) for s in range(S)}) > 1
        said = [m for m in _msgs(caplog) if f"block width {L}" in m and "1 steps per sweep" in m]
        assert len(said) == 2 * S and all(" sample_tau 0.5 seeds [0x" in m for m in said)
        if order == "sequential":
            assert all("layout interleaved" in m for m in said)
    finally:
        runtime.evict()


def test_engine_group_splits_on_group_boundaries_only():
    from conzic_amd import blocks as B_, harness, lengths, native
    from conzic_amd.engine import Engine, EngineGroup
    su = harness.build_synthetic(True, native.PREC_F32)
    eng = su.engine
    emb = np.random.default_rng(3).standard_normal((2, su.clip_cfg.proj)).astype(np.float32)
    eng.set_image_embeds(emb)
    try:
        W, n_cap = 3, 5
        one, nb = B_.tied_positions([B_.sequential_order(6, W, "interleaved")] * 2, W)
        groups, _, ior = B_.tied_rows(n_cap, W, image_of_caption=[0, 1, 0, 1, 1])
        pos = B_.caption_positions([one] * n_cap)
        perm = np.random.default_rng(8).permutation(n_cap * W)        # the rows of a group lie scattered
        groups, ior, pos = groups[perm], ior[perm], np.ascontiguousarray(pos[:, perm])
        start = lengths.length_rows(su.bert_tok, PROMPT, [6] * (n_cap * W))
        hps = [Engine.hyper(0.02, 2.0, 0.1) for _ in range(n_cap * W)]
        ids, cos = eng.generate_rows_tied(start, None, 4, K, pos, hps, None, groups, image_of_row=ior, snapshot_every=nb)
        grp = EngineGroup(eng, streams=2, min_images=3)
        try:
            grp.set_image_embeds(emb)
            parts = grp.tied_parts(groups)
            assert len(parts) == 2 and sorted(np.concatenate(parts).tolist()) == list(range(n_cap * W))
            assert not set(groups[parts[0]].tolist()) & set(groups[parts[1]].tolist())      # no group is cut
            idsg, cosg = grp.generate_rows_tied(start, None, 4, K, pos, hps, None, groups, image_of_row=ior, snapshot_every=nb)
            np.testing.assert_array_equal(idsg, ids)
            assert np.abs(cosg.astype(np.float64) - cos).max() <= 2e-6
        finally:
            grp.close(parent=False)
            eng.set_image_embeds(emb)
    finally:
        eng.close()


def test_demo_cli_block_width_zero(monkeypatch, caplog):
    from conzic_amd import demo_cli, runtime
    monkeypatch.setenv("CZC_PRECISION", "bf16")
    argv = ["--synthetic", "--tiny", "--run_type", "caption", "--order", "sequential", "--samples_num", "2", "--sentence_len", "5",
            "--num_iterations", "2", "--candidate_k", "50", "--block_width", "0"]
    try:
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            finals = demo_cli.main(argv)
    finally:
        runtime.evict()
    msgs = _msgs(caplog)
    assert len(finals) == 1 and len(finals[0]) == 2
    assert sum(m.startswith("final caption: ") for m in msgs) == 2
    assert sum(m.startswith("Order:sequential (block width 5, layout interleaved, 1 steps per sweep instead of 5)") for m in msgs) == 2


def test_out_of_scope_combinations_are_refused(capsys):
    from conzic_amd import demo_cli
    base = ["--synthetic", "--tiny", "--block_width", "2", "--order", "sequential"]
    for extra in (["--sentence_lens", "4,6"], ["--signals", "caption,positive"], ["--run_type", "infill", "--caption", "a _ dog"],
                  ["--run_type", "retrieve", "--index_captions", "captions.txt"], ["--run_type", "caption", "--order", "span"],
                  ["--run_type", "caption", "--order", "random"]):
        with pytest.raises(SystemExit):
            demo_cli.get_args(base + extra)
        assert "--block_width" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        demo_cli.get_args(["--synthetic", "--block_width", "-1"])
    a = demo_cli.get_args(["--synthetic", "--tiny", "--block_width", "0", "--block_layout", "contiguous", "--batch_samples",
                           "--sample_tau", "0.5"])
    assert a.block_width == 0 and a.block_layout == "contiguous"
    assert demo_cli.get_args(["--synthetic"]).block_width == 1


def test_run_cli_writes_the_sample_loops_files_from_one_call(tmp_path, monkeypatch):
    """--block_width 3 under --sample_tau (seeds by image name and sample): the sample loop and --batch_samples write the same
    files, in the layout of a run without the flag."""
    import json
    import os
    from PIL import Image
    from conzic_amd import run_cli, runtime, synth
    monkeypatch.setenv("CZC_PRECISION", "f32")
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    for j, u in enumerate(synth.make_images_u8(4, 40)):
        Image.fromarray(u).save(img_dir / f"im{j}.png")
    outs = []
    for extra in ([], ["--batch_samples"]):
        out_dir = tmp_path / ("rows" if extra else "loop")
        out_dir.mkdir()
        monkeypatch.chdir(out_dir)
        try:
            run_cli.main(["--synthetic", "--tiny", "--caption_img_path", str(img_dir), "--batch_size", "2", "--samples_num", "2",
                          "--run_type", "caption", "--order", "sequential", "--sentence_len", "5", "--candidate_k", "50",
                          "--num_iterations", "2", "--sample_tau", "0.5", "--block_width", "3"] + extra)
        finally:
            runtime.evict()
        files = {}
        for root, _, fs in os.walk(out_dir / "results"):
            for f in fs:
                files[os.path.relpath(os.path.join(root, f), out_dir)] = json.load(open(os.path.join(root, f)))
        outs.append(files)
    assert outs[0] == outs[1]
    assert len(outs[0]) == 2 * 3 and all(len(v) == 4 for v in outs[0].values())   # two samples x (two sweeps + best), four images
    assert {os.path.basename(k) for k in outs[0]} == {"iter_0.json", "iter_1.json", "best_clipscore.json"}


def test_control_tables_polish_blocks_and_the_exact_scorer_falls_back(monkeypatch, caplog):
    from conzic_amd import control, demo_cli, runtime
    monkeypatch.setenv("CZC_PRECISION", "f32")
    argv = ["--synthetic", "--tiny", "--run_type", "controllable", "--control_type", "sentiment", "--order", "sequential",
            "--samples_num", "1", "--sentence_len", "5", "--num_iterations", "2", "--candidate_k", "50", "--control_scores", "table",
            "--block_width", "2", "--block_layout", "contiguous"]
    try:
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            demo_cli.main(argv)
        msgs = _msgs(caplog)
        assert sum("block width 2, layout contiguous, 3 steps per sweep instead of 5" in m for m in msgs) == 1
        assert sum(m.startswith("final caption: ") for m in msgs) == 1
        runtime.evict()
        caplog.clear()
        real = control.configure
        monkeypatch.setattr(control, "configure", lambda *a, **k: real(*a, **k) and "exact")   # tables set, reported as the callback
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            demo_cli.main(argv)
        msgs = _msgs(caplog)
        assert sum("falling back to block width 1" in m for m in msgs) == 1
        assert not any("steps per sweep" in m for m in msgs)
        assert sum(m.startswith("final caption: ") for m in msgs) == 1
    finally:
        runtime.evict()
