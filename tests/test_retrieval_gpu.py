"""-m gpu: caption retrieval through the user layer on the tiny engine -- retrieval.TextIndex, the drop-in clip/clipretrieval.py
`CLIPIndex` against the golden recorded from the reference's own class, runtime.retrieve_then_polish and `--run_type retrieve`
of the CLI."""
import json
import logging
import os

import numpy as np
import pytest

import retrieval_ref as ref
from conzic_amd import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 2e-6          # on a cosine against fp64 (tests/test_index_search_gpu.py)
PROMPT = "Image of a"


def _captions(sv, n, seed):
    words = sv.bert_tokens[sv.regular_lo:sv.regular_hi]
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = " ".join(words[i] for i in rng.integers(0, len(words), size=int(rng.integers(3, 9))))
        if c not in out:
            out.append(c)
    return out


@pytest.fixture()
def models(monkeypatch):
    """Tiny synthetic LM / CLIP / tokenizer objects as the drop-in modules take them, on the split-fp16 engine."""
    from clip.clip import CLIP
    from conzic_amd import runtime
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab
    from PIL import Image
    monkeypatch.setenv("CZC_PRECISION", "split")
    monkeypatch.delenv("CZC_MEMO_ROWS", raising=False)
    sv = synth.make_vocab_tiny()
    bcfg, ccfg = synth.bert_tiny(len(sv.bert_tokens)), synth.clip_tiny(len(sv.clip_vocab))
    bt, ct = tokenizers_from_vocab(sv)
    lm = SyntheticLM(bcfg)
    clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, 12), ct)
    imgs = [Image.fromarray(u) for u in synth.make_images_u8(2, ccfg.v_image)]
    yield sv, bt, lm, clip, imgs
    runtime.evict()


def test_text_index_from_captions_and_search(models):
    from conzic_amd.retrieval import TextIndex
    sv, bt, lm, clip, imgs = models
    caps = _captions(sv, 200, 1)
    index = TextIndex.from_captions(clip, caps, chunk=64)
    assert len(index) == 200 and index.matrix.shape == (200, 64) and index.captions == caps
    hits = index.search(clip, imgs, 5)
    emb = clip.last_image_embeds()                 # the embeddings the engine itself returned
    assert emb.shape == (2, 64) and len(hits) == 2 and all(len(h) == 5 for h in hits)
    sc = ref.scores(emb, index.matrix)
    r_ids, r_cos = ref.search(emb, index.matrix, 6)
    worst = 0.0
    for b in range(2):
        for j, (caption, cosine, row) in enumerate(hits[b]):
            assert caption == caps[row]
            err = max(abs(cosine - r_cos[b, j]), abs(cosine - sc[b, row]))
            worst = max(worst, err)
            assert err <= BAR, (b, j, err)
            if r_cos[b, j] - r_cos[b, j + 1] > 2 * BAR and (j == 0 or r_cos[b, j - 1] - r_cos[b, j] > 2 * BAR):
                assert row == r_ids[b, j], (b, j)
    print(f"TextIndex.search: worst |cosine - fp64| {worst:.3e} (bar {BAR:.0e})")
    assert clip._eng().index_size() == 200
    index.attach(clip._eng())                      # a second attach of the same index sets nothing
    ids2, cos2 = index.search_ids(clip, imgs, 5)
    assert [[h[2] for h in per] for per in hits] == ids2.tolist()


def test_drop_in_clip_index_returns_the_golden_captions(models, tmp_path):
    """clip/clipretrieval.py over the golden's files and images: the captions the reference's own CLIPIndex returned."""
    from PIL import Image
    from clip.clipretrieval import CLIPIndex
    sv, bt, lm, clip, imgs = models
    z = np.load(os.path.join(GOLDEN, "retrieval_tiny.npz"))
    with open(os.path.join(GOLDEN, "retrieval_tiny.json"), encoding="utf8") as f:
        meta = json.load(f)
    assert min(meta["margins"]) > 1e-3
    mpath, dpath = str(tmp_path / "index.txt"), str(tmp_path / "mapping.json")
    with open(mpath, "w", encoding="utf8") as f:
        for row in z["index_matrix"]:
            f.write(" ".join("%.9g" % v for v in row) + "\n")
    with open(dpath, "w", encoding="utf8") as f:
        json.dump(meta["mapping"], f)
    index = CLIPIndex(mpath, dpath, clip)
    assert index.mapping_dict == meta["mapping"] and index.index_matrix.shape == (257, 64)
    for j, u8 in enumerate(z["images_u8"]):
        ipath = str(tmp_path / f"img{j}.png")
        Image.fromarray(u8).save(ipath)
        assert index.search_text(ipath) == meta["winners"][j], j
        vec = index.get_image_representation(ipath)
        assert vec.shape == (1, 64) and abs(float(np.linalg.norm(vec)) - 1.0) < 1e-5
        want = z["image_embeds"][j] / np.linalg.norm(z["image_embeds"][j])
        assert np.abs(vec[0] - want).max() < 1e-4          # the vision tower's own parity is tests/test_step_gpu.py's subject


def test_retrieve_then_polish_is_run_infill_on_the_retrieved_captions(models, monkeypatch):
    """For its drafts, retrieve_then_polish returns what run_infill called directly with those captions and image_of_caption
    returns: ids and cosines bit for bit."""
    from clip.clip import ImageEmbeds
    from conzic_amd import runtime
    from conzic_amd.retrieval import TextIndex
    sv, bt, lm, clip, imgs = models
    log = logging.getLogger("retrieval-test")
    caps = _captions(sv, 60, 2)
    index = TextIndex.from_captions(clip, caps)
    snaps = []
    real = runtime._bookkeeping

    def spy(order, ids, cos, *a, **k):
        snaps.append((np.array(ids), np.array(cos)))
        return real(order, ids, cos, *a, **k)

    monkeypatch.setattr(runtime, "_bookkeeping", spy)
    kw = dict(order="sequential", max_iters=2, top_k=50, temperature=0.1, alpha=0.02, beta=2.0)

    def mask():
        m = synth.make_token_mask(sv)
        m[:, bt.mask_token_id] = 0
        return m

    names = ["img0", "img1"]
    out = runtime.retrieve_then_polish(index, names, lm, clip, bt, imgs, mask(), PROMPT, log, k=3, **kw)
    assert len(out) == 2 and all(len(o["retrieved"]) == 3 for o in out)
    drafts = [o["retrieved"][j][0] for o in out for j in o["drafts"]]
    ioc = [b for b, o in enumerate(out) for _ in o["drafts"]]
    assert len(drafts) >= 4 and len(snaps) == len(drafts)
    via_retrieval = list(snaps)
    del snaps[:]
    emb = clip.last_image_embeds()
    direct = runtime.run_infill(drafts, names, lm, clip, bt, ImageEmbeds(emb), mask(), PROMPT, log, positions="all",
                                image_of_caption=ioc, **kw)
    assert len(snaps) == len(drafts)
    for (i0, c0), (i1, c1) in zip(via_retrieval, snaps):
        np.testing.assert_array_equal(i0, i1)
        np.testing.assert_array_equal(c0.view(np.uint32), c1.view(np.uint32))
    polished = [p for o in out for p in o["polished"]]
    assert [p[0] for p in polished] == [d[0] for d in direct] and [p[1] for p in polished] == [d[1] for d in direct]
    # the retrieved cosines are the index search's own
    ids, cos = index.search_ids(clip, ImageEmbeds(emb), 3)
    assert [[h[2] for h in o["retrieved"]] for o in out] == ids.tolist()
    assert [[h[1] for h in o["retrieved"]] for o in out] == cos.astype(np.float64).tolist()


@pytest.mark.parametrize("polish", [False, True])
def test_demo_cli_retrieve(polish, tmp_path, caplog):
    """`demo_cli --synthetic --tiny --run_type retrieve --index_captions FILE [--polish]` runs and logs what it found."""
    from conzic_amd import demo_cli, runtime
    caps = _captions(synth.make_vocab_tiny(), 40, 3)
    path = tmp_path / "captions.txt"
    path.write_text("\n".join(caps) + "\n", encoding="utf8")
    argv = ["--synthetic", "--tiny", "--run_type", "retrieve", "--index_captions", str(path), "--retrieve_k", "2",
            "--batch_size", "2", "--order", "sequential", "--num_iterations", "2", "--candidate_k", "20"]
    try:
        with caplog.at_level(logging.INFO, logger="ConZIC"):
            demo_cli.main(argv + (["--polish"] if polish else []))
    finally:
        runtime.evict()
    lines = [r.getMessage() for r in caplog.records]
    found = [ln for ln in lines if ", retrieved " in ln and "clip score" in ln]
    assert len(found) == 4 and all(ln.split(": ", 2)[-1] in caps for ln in found), lines[-10:]
    assert any(ln.startswith("text index: 40 captions x 64") for ln in lines)
    assert sum(ln.startswith("final caption: ") for ln in lines) == (4 if polish else 0)
    assert sum(ln.startswith("best caption: ") for ln in lines) == (4 if polish else 0)
