"""conzic_amd.vocab on the host: bitsets, word lists, the runtime's refusal of a short allow-list, and the command-line flags."""
import logging

import numpy as np
import pytest

from conzic_amd import demo_cli, run_cli, runtime, synth, vocab
from conzic_amd.text import tokenizers_from_vocab


@pytest.fixture(scope="module")
def tok():
    sv = synth.make_vocab_tiny()
    return tokenizers_from_vocab(sv)[0], synth.make_token_mask(sv).reshape(-1)


def test_library_exports_the_call_and_the_version():
    from conzic_amd import native
    lib = native.load()
    assert lib.czc_version() >= 108
    assert hasattr(lib, "czc_generate_rows_vocab") and hasattr(native.load_test(), "czc_test_topk_rows_vocab")
    assert native.MAX_VOCAB_SETS == 4096


def _reference_bits(masks, V):
    """bit by bit: word i >> 5, bit i & 31"""
    out = np.zeros((len(masks), (V + 31) // 32), dtype=np.uint32)
    for n, m in enumerate(masks):
        for i in range(V):
            if m[i]:
                out[n, i >> 5] = int(out[n, i >> 5]) | (1 << (i & 31))
    return out


@pytest.mark.parametrize("V", [1, 31, 32, 33, 30522])
def test_pack_against_a_bit_by_bit_reference(V):
    rng = np.random.default_rng(V)
    masks = [rng.random(V) < 0.5, np.ones(V, bool), np.zeros(V, bool), np.arange(V) == V - 1]
    bits = vocab.pack(masks, V)
    assert bits.dtype == np.uint32 and bits.shape == (4, (V + 31) // 32)
    np.testing.assert_array_equal(bits, _reference_bits(masks, V))
    np.testing.assert_array_equal(vocab.pack([np.nonzero(m)[0] for m in masks], V), bits)   # id lists, the same sets
    np.testing.assert_array_equal(vocab.unpack(bits, V), np.stack(masks))
    if V % 32:   # nothing at or above V is ever set
        assert int(bits[1, -1]) == (1 << (V % 32)) - 1
    for bad in ([V], [-1]):
        with pytest.raises(ValueError):
            vocab.pack([bad], V)
    with pytest.raises(ValueError):
        vocab.pack([np.ones(V + 1, bool)], V)


def _words(tok_mask, n):
    """n regular single-token words the token mask lets through"""
    t, mask = tok_mask
    out = []
    for i in np.nonzero(mask > 0)[0]:
        w = t.id2tok[int(i)]
        if w.isalpha() and w.isascii() and vocab.token_ids(t, [w])[0] == [int(i)]:
            out.append(w)
        if len(out) == n:
            break
    assert len(out) == n
    return out


def test_ban_and_allow(tok, caplog):
    t, mask = tok
    V = t.vocab_size
    w = _words(tok, 3)
    ids = [t.vocab[x] for x in w]
    two_pieces = w[0] + w[1]
    assert two_pieces not in t.vocab
    with caplog.at_level(logging.INFO, logger="ConZIC"):
        bits, skipped = vocab.ban(t, [w[0], two_pieces, "¤¤", w[2], "[MASK]", ""])
    assert skipped == [two_pieces, "¤¤", "[MASK]", ""]
    assert any("skipped" in r.getMessage() and two_pieces in r.getMessage() for r in caplog.records)   # never silently dropped
    allowed = vocab.unpack(bits, V)
    assert not allowed[ids[0]] and not allowed[ids[2]] and allowed[ids[1]] and allowed.sum() == V - 2
    dot = t.vocab["."]
    bits, skipped = vocab.allow(t, [w[0], w[1], two_pieces])
    assert skipped == [two_pieces]
    assert sorted(np.nonzero(vocab.unpack(bits, V))[0].tolist()) == sorted([ids[0], ids[1], dot])
    bits, _ = vocab.allow(t, [w[0], w[1]], keep_dot=False)
    assert sorted(np.nonzero(vocab.unpack(bits, V))[0].tolist()) == sorted(ids[:2])


def test_effective_size(tok):
    t, mask = tok
    V = t.vocab_size
    w = _words(tok, 2)
    stop = int(np.nonzero(mask == 0)[0][-1])
    sets = vocab.pack([[t.vocab[w[0]], t.vocab[w[1]], stop], np.ones(V, bool), []], V)
    np.testing.assert_array_equal(vocab.effective_size(sets, mask), [2, int((mask != 0).sum()), 0])
    assert vocab.effective_size(sets[0], mask) == 2
    assert vocab.effective_size(vocab.ban(t, w)[0], mask) == int((mask != 0).sum()) - 2


def test_runtime_refuses_an_allow_list_below_top_k(tok):
    t, mask = tok
    w = _words(tok, 6)
    short = vocab.Vocab(vocab.allow(t, w)[0], allow_list=True)
    assert short.check(mask, 6).tolist() == [6]       # the six words; '.' is a stop word of the mask
    with pytest.raises(ValueError) as exc:
        short.check(mask, 7)
    assert "--candidate_k" in str(exc.value) and "widen the list" in str(exc.value)
    # run_generation_samples refuses before it builds an engine (no model, no GPU needed to get here)
    with pytest.raises(ValueError) as exc:
        runtime.run_generation_samples("sequential", 2, ["img0"], None, None, t, None, mask[None, :], "Image of a", logging.getLogger("ConZIC"),
                                       5, 50, 0.1, 0.02, 2.0, 2, 1, vocab=short)
    assert "--candidate_k" in str(exc.value)
    # a ban-list is never refused for its size, and the sets of samples beyond the table are
    vocab.Vocab(vocab.ban(t, w)[0]).check(mask, 500)
    per = vocab.Vocab(vocab.pack([np.ones(t.vocab_size, bool)] * 3, t.vocab_size))
    assert per.set_of_sample(2, sample0=1).tolist() == [1, 2]
    with pytest.raises(ValueError):
        per.set_of_sample(4)
    assert vocab.Vocab(vocab.ban(t, w)[0]).set_of_sample(4).tolist() == [0, 0, 0, 0]


def test_cli_flags_and_refused_combinations(tmp_path, capsys):
    assert run_cli.get_args is demo_cli.get_args
    a = demo_cli.get_args(["--synthetic"])
    assert a.ban_words is None and a.allow_words is None and a.ban_per_sample is None and not vocab.wanted(a)
    a = demo_cli.get_args(["--synthetic", "--ban_words", "a,b", "--allow_words", "c,d", "--batch_samples", "--sample_tau", "0.5",
                           "--distinct", "1.0", "--batch_size", "2"])
    assert a.ban_words == "a,b" and a.allow_words == "c,d" and vocab.wanted(a)
    for flag in (["--ban_words", "a"], ["--allow_words", "a"]):
        for extra in (["--sentence_lens", "4,6"], ["--signals", "caption,positive"], ["--block_width", "2", "--order", "sequential"],
                      ["--run_type", "infill", "--caption", "a _ dog"], ["--run_type", "retrieve", "--index_captions", "captions.txt"]):
            with pytest.raises(SystemExit):
                demo_cli.get_args(["--synthetic", "--order", "sequential"] + flag + extra)
            err = capsys.readouterr().err
            assert "--ban_words / --allow_words" in err and "command-line plumbing does not yet" in err
    # a file with one word per line, or a comma-separated list
    f = tmp_path / "words.txt"
    f.write_text("red\n\n green \nblue\n")
    assert vocab.parse_words(str(f)) == ["red", "green", "blue"]
    assert vocab.parse_words("red, green,,blue") == ["red", "green", "blue"]


def test_ban_per_sample_parsing(tok, tmp_path, capsys):
    t, mask = tok
    w = _words(tok, 3)
    f = tmp_path / "per_sample.txt"
    f.write_text(f"{w[0]}\n{w[1]}, {w[2]}\n\n")
    assert vocab.parse_per_sample(str(f)) == [[w[0]], [w[1], w[2]], []]
    base = ["--synthetic", "--ban_per_sample", str(f)]
    with pytest.raises(SystemExit):
        demo_cli.get_args(base + ["--samples_num", "3"])
    assert "requires --batch_samples" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        demo_cli.get_args(base + ["--batch_samples", "--samples_num", "2"])
    assert "3 lines for --samples_num 2" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        demo_cli.get_args(["--synthetic", "--batch_samples", "--ban_per_sample", str(tmp_path / "missing.txt")])
    assert "no such file" in capsys.readouterr().err
    a = demo_cli.get_args(base + ["--batch_samples", "--samples_num", "3", "--ban_words", w[0]])
    v = vocab.from_arguments(a, t)
    allowed = vocab.unpack(v.bits, t.vocab_size)
    assert v.bits.shape[0] == 3 and not v.allow_list
    ids = [t.vocab[x] for x in w]
    assert not allowed[:, ids[0]].any()                                   # --ban_words holds for every sample
    assert allowed[0, ids[1]] and not allowed[1, ids[1]] and not allowed[1, ids[2]] and allowed[2, ids[1]] and allowed[2, ids[2]]
    assert v.set_of_sample(3).tolist() == [0, 1, 2]
    assert vocab.from_arguments(demo_cli.get_args(["--synthetic"]), t) is None
    one = vocab.from_arguments(demo_cli.get_args(["--synthetic", "--allow_words", ",".join(w), "--ban_words", w[0]]), t)
    assert one.allow_list and one.bits.shape[0] == 1
    assert sorted(np.nonzero(vocab.unpack(one.bits, t.vocab_size)[0])[0].tolist()) == sorted([ids[1], ids[2], t.vocab["."]])


def test_a_wrong_size_set_of_row_is_refused_by_name_before_the_library():
    from conzic_amd.engine import Engine
    eng = Engine.__new__(Engine)   # no library, no handle
    kw = dict(init_rows=np.zeros((3, 9), np.int32), lens=[2, 3, 4], seed_len=4, top_k=8, positions=np.zeros((4, 3), np.int32),
              hypers=[Engine.hyper(0.02, 2.0, 0.1) for _ in range(3)])
    for bad in ([0, 1], [0, 0, 1, 1]):
        with pytest.raises(ValueError) as ei:
            eng.generate_rows_vocab(set_of_row=bad, **kw)
        assert str(ei.value).startswith("generate_rows_vocab:") and "set_of_row" in str(ei.value)
