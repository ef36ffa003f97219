"""-m gpu: --ban_words / --ban_per_sample of the CLIs (conzic_amd.vocab, runtime.run_generation_samples on
czc_generate_rows_vocab), on the tiny synthetic towers: the captions lack the words, they are the captions of the same run under
a token mask with the words removed by hand, and every sample of a batched call keeps to its own list."""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BASE = ["--synthetic", "--tiny", "--run_type", "caption", "--order", "sequential", "--batch_samples", "--samples_num", "4",
        "--sentence_len", "5", "--num_iterations", "2", "--candidate_k", "50"]


def _run(argv, caplog=None):
    """-> (the final caption of every sample of the one image, the log lines; none without caplog)"""
    from conzic_amd import demo_cli, runtime
    try:
        if caplog is None:
            return demo_cli.main(argv)[0], []
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            finals = demo_cli.main(argv)
    finally:
        runtime.evict()
    return finals[0], [r.getMessage() for r in caplog.records]


def _tokenizer():
    from conzic_amd import synth
    from conzic_amd.text import tokenizers_from_vocab
    sv = synth.make_vocab_tiny()
    return tokenizers_from_vocab(sv)[0], synth.make_token_mask(sv)


N_PROMPT = 3   # "image of a": the prompt leads every caption and is never polished


def _said(caption):
    """the words a caption says behind its prompt"""
    return caption.split()[N_PROMPT:]


def _bannable(caption):
    """the polished words of a caption that are single regular tokens the token mask lets through"""
    from conzic_amd import vocab
    tok, mask = _tokenizer()
    out = []
    for w in _said(caption):
        ids, _ = vocab.token_ids(tok, [w])
        if ids and w != "." and mask.reshape(-1)[ids[0]] != 0 and w not in out:
            out.append(w)
    return out


@pytest.fixture(scope="module")
def free_caption():
    """the caption of the run without word lists (sequential order and argmax: the same for every sample)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("CZC_PRECISION", "bf16")
    try:
        finals, _ = _run(BASE)
    finally:
        mp.undo()
    assert len(finals) == 4 and len(set(finals)) == 1
    words = _bannable(finals[0])
    assert len(words) >= 2, finals[0]
    return finals[0], words


def test_banned_words_stay_out_and_equal_the_premultiplied_mask(free_caption, monkeypatch, caplog):
    from conzic_amd import synth, vocab
    monkeypatch.setenv("CZC_PRECISION", "bf16")
    caption, words = free_caption
    finals, msgs = _run(BASE + ["--ban_words", ",".join(words[:2]) + ",notaword"], caplog)
    assert len(finals) == 4
    for c in finals:
        assert not set(_said(c)) & set(words[:2]), (c, words[:2])
    assert finals[0] != caption
    said = [m for m in msgs if "vocab sets: 0: " in m]
    assert len(said) == 4 and all("skipped ['notaword']" in m for m in said)
    # the same run with the words taken out of the token mask by hand, through the call that knows no sets
    tok, _ = _tokenizer()
    bits, skipped = vocab.ban(tok, words[:2])
    assert not skipped
    real = synth.make_token_mask
    monkeypatch.setattr(synth, "make_token_mask", lambda sv, **kw: (real(sv, **kw) * vocab.unpack(bits, tok.vocab_size)).astype(np.float32))
    by_hand, msgs = _run(BASE, caplog)
    assert not any("vocab sets" in m for m in msgs)
    assert by_hand == finals


def test_ban_per_sample(free_caption, monkeypatch, caplog, tmp_path):
    monkeypatch.setenv("CZC_PRECISION", "bf16")
    caption, words = free_caption
    lists = [[words[0]], [words[1]], [], [words[0], words[1]]]
    f = tmp_path / "per_sample.txt"
    f.write_text("\n".join(",".join(ws) for ws in lists) + "\n")
    finals, msgs = _run(BASE + ["--ban_per_sample", str(f)], caplog)
    assert len(finals) == 4
    for c, ws in zip(finals, lists):
        assert not set(_said(c)) & set(ws), (c, ws)
    assert finals[2] == caption and finals[0] != caption and finals[1] != caption
    assert sum("vocab sets: " in m for m in msgs) == 4
    # sample 0 alone with its list
    f1 = tmp_path / "one.txt"
    f1.write_text(words[0] + "\n")
    one, _ = _run([a if a != "4" else "1" for a in BASE] + ["--ban_per_sample", str(f1)], caplog)
    assert one == finals[:1]
