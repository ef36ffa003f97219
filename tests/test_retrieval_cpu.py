"""Caption retrieval without a GPU: the fp64 reference of the search against the golden recorded from the reference's own
CLIPIndex (tests/golden/make_retrieval_goldens.py), the index files, the C ABI's declarations, the CLI switches and the
rule by which retrieve_then_polish skips captions that cannot be drafts."""
import json
import logging
import os
import re

import numpy as np
import pytest

import retrieval_ref as ref
from conzic_amd import demo_cli, native
from conzic_amd.retrieval import TextIndex

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "retrieval_tiny.npz"))
    with open(os.path.join(GOLDEN, "retrieval_tiny.json"), encoding="utf8") as f:
        meta = json.load(f)
    return z, meta


def _write_reference_files(tmp_path, z, meta):
    """The index as the reference's clip/build_text_index.py writes it: one row of space-separated floats per line + JSON."""
    mpath, dpath = str(tmp_path / "index.txt"), str(tmp_path / "mapping.json")
    with open(mpath, "w", encoding="utf8") as f:
        for row in z["index_matrix"]:
            f.write(" ".join("%.9g" % v for v in row) + "\n")
    with open(dpath, "w", encoding="utf8") as f:
        json.dump(meta["mapping"], f)
    return mpath, dpath


def test_reference_reproduces_the_golden(golden):
    z, meta = golden
    X, emb, want = z["index_matrix"], z["image_embeds"], z["scores"]
    assert X.shape == (257, 64) and X.dtype == np.float32 and emb.shape == (3, 64) and want.shape == (3, 257)
    got = ref.scores(emb, X)
    assert np.abs(got - want).max() <= 1e-12
    ids, cos = ref.search(emb, X, 5)
    for j in range(3):
        assert meta["mapping"][str(int(ids[j, 0]))] == meta["winners"][j]
        assert abs(cos[j, 0] - want[j].max()) <= 1e-12
        assert cos[j, 0] - cos[j, 1] > 1e-3          # the generator's promise: every winner leads by more than 1e-3
        assert (np.diff(cos[j]) <= 0).all()
    assert len(set(meta["winners"])) == 3


def test_reference_orders_ties_by_id_and_pads_the_tail():
    X = np.array([[1, 0], [0, 1], [2, 0], [1, 1]], dtype=np.float32)
    ids, cos = ref.search(np.array([[3, 0]], dtype=np.float32), X, 6)
    assert ids.tolist() == [[0, 2, 3, 1, -1, -1]]
    assert cos[0, 0] == cos[0, 1] == 1.0 and np.isneginf(cos[0, 4:]).all()


def test_text_index_files(golden, tmp_path):
    z, meta = golden
    mpath, dpath = _write_reference_files(tmp_path, z, meta)
    index = TextIndex.load(mpath, dpath)
    assert len(index) == 257 and index.matrix.dtype == np.float32
    np.testing.assert_array_equal(index.matrix, z["index_matrix"])
    assert index.captions == [meta["mapping"][str(i)] for i in range(257)]
    for name in ("again.txt", "again.npy"):           # save -> load round-trips, text and .npy
        m2, d2 = str(tmp_path / name), str(tmp_path / (name + ".json"))
        index.save(m2, d2)
        back = TextIndex.load(m2, d2)
        np.testing.assert_array_equal(back.matrix, index.matrix)
        assert back.captions == index.captions
    with open(str(tmp_path / "again.txt"), encoding="utf8") as f:
        first = f.readline()
    assert len(first.split()) == 64 and "\t" not in first and "," not in first
    with open(dpath, "w", encoding="utf8") as f:
        json.dump({k: v for k, v in meta["mapping"].items() if k != "7"}, f)
    with pytest.raises(ValueError):
        TextIndex.load(mpath, dpath)
    with pytest.raises(ValueError):
        TextIndex(z["index_matrix"], ["one caption"])


def test_c_abi_declares_the_index_functions():
    with open(native.HEADER_PATH, encoding="utf8") as f:
        header = f.read()
    for name, args in (("czc_index_set", r"czc_engine\* e, const float\* embeds, int64_t n"),
                       ("czc_index_size", r"czc_engine\* e, int64_t\* n"),
                       ("czc_index_search", r"czc_engine\* e, const float\* image_embeds, int Q, int k, int32_t\* out_ids, float\* out_cos")):
        assert re.search(r"\bint " + name + r"\(" + args + r"\);", header), name
        assert name in native.SIGNATURES
    assert re.search(r"#define CZC_INDEX_MAX_K 64\b", header) and native.INDEX_MAX_K == 64
    assert re.search(r"#define CZC_MAX_BERT_LEN %d\b" % native.MAX_BERT_LEN, header)
    import ctypes as C
    assert native.SIGNATURES["czc_index_set"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64])
    assert native.SIGNATURES["czc_index_search"][1] == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib = native.load()
    assert lib.czc_version() >= 103
    for name in ("czc_index_set", "czc_index_size", "czc_index_search"):
        assert hasattr(lib, name)


BASE = ["--synthetic", "--tiny", "--run_type", "retrieve"]


def test_cli_accepts_the_retrieve_switches():
    a = demo_cli.get_args(BASE + ["--index_matrix_path", "m.txt", "--mapping_dict_path", "d.json"])
    assert a.run_type == "retrieve" and a.retrieve_k == 1 and not a.polish and a.index_captions is None
    a = demo_cli.get_args(BASE + ["--index_captions", "caps.txt", "--retrieve_k", "5", "--polish", "--order", "sequential"])
    assert a.index_captions == "caps.txt" and a.retrieve_k == 5 and a.polish
    a = demo_cli.get_args(["--synthetic", "--tiny"])       # the switches default to off
    assert a.run_type == "controllable" and not a.polish and a.index_matrix_path is None and a.index_captions is None


@pytest.mark.parametrize("argv", [
    BASE,                                                                         # no index at all
    BASE + ["--index_matrix_path", "m.txt"],                                      # half of the pair
    BASE + ["--mapping_dict_path", "d.json"],
    BASE + ["--index_matrix_path", "m.txt", "--mapping_dict_path", "d.json", "--index_captions", "c.txt"],
    BASE + ["--index_captions", "c.txt", "--retrieve_k", "0"],
    BASE + ["--index_captions", "c.txt", "--retrieve_k", "65"],
    BASE + ["--index_captions", "c.txt", "--polish", "--order", "span"],
    BASE + ["--index_captions", "c.txt", "--polish", "--order", "random"],
    BASE + ["--index_captions", "c.txt", "--sentence_lens", "4,6"],
    BASE + ["--index_captions", "c.txt", "--signals", "caption,positive"],
    BASE + ["--index_captions", "c.txt", "--caption", "a _ dog"],
    ["--synthetic", "--tiny", "--run_type", "caption", "--polish"],               # the switches belong to retrieve
    ["--synthetic", "--tiny", "--run_type", "caption", "--index_captions", "c.txt"],
])
def test_cli_rejects(argv, capsys):
    with pytest.raises(SystemExit) as ei:
        demo_cli.get_args(argv)
    assert ei.value.code == 2
    assert "error:" in capsys.readouterr().err


class _StubIndex:
    def __init__(self, hits):
        self.hits = hits

    def search(self, clip, images, k):
        return [per_image[:k] for per_image in self.hits]


class _StubClip:
    """What retrieve_then_polish touches of a CLIP wrapper when the index and run_infill are stand-ins: no engine behind it."""

    def last_image_embeds(self):
        return np.ones((2, 64), dtype=np.float32)


def test_retrieve_then_polish_skips_what_cannot_be_a_draft(monkeypatch, caplog):
    from conzic_amd import harness, runtime
    from conzic_amd.text import tokenizers_from_vocab
    bt, _ = tokenizers_from_vocab(harness.cached_vocab(True))
    prompt = "Image of a"
    seed_tokens = len(bt.encode(prompt))                       # [CLS] + prompt + [SEP]
    fits = " ".join(["picture"] * (native.MAX_BERT_LEN - seed_tokens))
    too_long = fits + " picture"
    assert runtime.draft_skip_reason(bt, prompt, "the picture of photos") is None
    assert runtime.draft_skip_reason(bt, prompt, fits) is None
    assert "more than" in runtime.draft_skip_reason(bt, prompt, too_long)
    assert runtime.draft_skip_reason(bt, prompt, "") == "empty after tokenising"
    assert runtime.draft_skip_reason(bt, prompt, "   ") == "empty after tokenising"
    hits = [[("the picture of photos", 0.5, 3), ("", 0.4, 9), (too_long, 0.3, 1)],
            [("   ", 0.6, 2), ("photo of the picture", 0.5, 0), (fits, 0.1, 8)]]
    calls = []

    def fake_run_infill(captions, img_name, model, clip, tokenizer, image_instance, token_mask, prompt_, logger, **kw):
        calls.append((list(captions), kw, image_instance))
        return [([[c + " (polished)"], [c + " (best)"]], [[0.7], [0.7]]) for c in captions]

    monkeypatch.setattr(runtime, "run_infill", fake_run_infill)
    log = logging.getLogger("retrieval-test")
    with caplog.at_level(logging.INFO, logger="retrieval-test"):
        out = runtime.retrieve_then_polish(_StubIndex(hits), ["img0", "img1"], None, _StubClip(), bt, object(), None, prompt, log,
                                           k=3, order="sequential", max_iters=2)
    (captions, kw, image_instance), = calls                    # ONE run_infill call over all drafts
    assert captions == ["the picture of photos", "photo of the picture", fits]
    assert kw["positions"] == "all" and kw["image_of_caption"] == [0, 1, 1] and kw["order"] == "sequential" and kw["max_iters"] == 2
    assert image_instance.embeds.shape == (2, 64)              # the images are not encoded a second time
    assert [o["drafts"] for o in out] == [[0], [1, 2]]
    assert [o["retrieved"] for o in out] == hits
    assert out[0]["polished"][0][0][-1] == ["the picture of photos (best)"] and len(out[1]["polished"]) == 2
    skipped = [r.getMessage() for r in caplog.records if "is not polished" in r.getMessage()]
    assert len(skipped) == 3 and sum("empty after tokenising" in m for m in skipped) == 2
    with pytest.raises(TypeError):
        runtime.retrieve_then_polish(_StubIndex(hits), ["img0", "img1"], None, _StubClip(), bt, object(), None, prompt, log,
                                     positions="blanks")
    # nothing that can be a draft: no run_infill call at all
    del calls[:]
    out = runtime.retrieve_then_polish(_StubIndex([[("", 0.1, 0)]]), ["img0"], None, _StubClip(), bt, object(), None, prompt, log)
    assert not calls and out == [dict(retrieved=[("", 0.1, 0)], drafts=[], polished=[])]
