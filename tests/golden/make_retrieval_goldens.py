#!/usr/bin/env python
"""Generate tests/golden/retrieval_tiny.{npz,json} by running the REAL reference's retrieval baseline.

Runs only where the reference checkout and `transformers` are (as make_goldens.py, whose shims and tiny-model builder it
imports unchanged); nothing here is used at test time and it is not a test.  The reference's `clip/clipretrieval.py::CLIPIndex`
is imported UNCHANGED (`progressbar`, which it imports and never uses in the class, is stubbed) and driven on the CPU with the
tiny synthetic CLIP: an index of 257 synthetic captions written in the reference's own text format, and 3 synthetic images
saved as files.  Recorded: the index matrix (fp32, as the text file holds it), the mapping, the images (uint8) and their
embeddings, `search_text`'s caption per image and the full fp64 score row per image.  The captions and images are drawn again
until every image has a winner of its own that leads the runner-up by more than 1e-3, which is asserted.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (path shims, stand-ins, build_hf; the reference becomes importable)
sys.path.remove(HERE)

sys.modules.setdefault("progressbar", types.SimpleNamespace(ProgressBar=lambda *a, **k: None))
import clip.clipretrieval as ref_retrieval  # noqa: E402  (reference)
assert ref_retrieval.__file__.startswith(mg.REF + "/"), ref_retrieval.__file__

from conzic_amd import synth  # noqa: E402

N_CAPTIONS, N_IMAGES, MARGIN = 257, 3, 1e-3


def make_captions(sv, rng):
    """N_CAPTIONS distinct sentences of 3..8 one-token words of the synthetic vocabulary."""
    words = sv.bert_tokens[sv.regular_lo:sv.regular_hi]
    seen, out = set(), []
    while len(out) < N_CAPTIONS:
        c = " ".join(words[i] for i in rng.integers(0, len(words), size=int(rng.integers(3, 9))))
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def make_images(S, rng):
    """N_IMAGES images that differ in colour and structure (pure noise images all land on one embedding): a colour gradient of
    random direction between two random colours, plus a little noise."""
    yy, xx = np.mgrid[0:S, 0:S] / max(S - 1, 1)
    out = []
    for _ in range(N_IMAGES):
        a, b = rng.integers(0, 256, size=3), rng.integers(0, 256, size=3)
        th = rng.uniform(0, 2 * np.pi)
        t = np.clip(0.5 + (np.cos(th) * (xx - 0.5) + np.sin(th) * (yy - 0.5)), 0, 1)[..., None]
        img = a * (1 - t) + b * t + rng.normal(0, 8, size=(S, S, 3))
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return np.stack(out)


def main():
    from PIL import Image
    sv = synth.make_vocab_tiny()
    bcfg, ccfg = synth.bert_tiny(len(sv.bert_tokens)), synth.clip_tiny(len(sv.clip_vocab))
    with tempfile.TemporaryDirectory() as tmp:
        _, _, clip = mg.build_hf(bcfg, ccfg, sv, 11, 12, tmp)
        for seed in range(100):
            rng = np.random.default_rng(seed)
            captions = make_captions(sv, rng)
            matrix = np.concatenate([clip.compute_batch_index_text_representation(captions[i:i + 64]).numpy()
                                     for i in range(0, N_CAPTIONS, 64)]).astype(np.float32)
            mpath, dpath = os.path.join(tmp, "index.txt"), os.path.join(tmp, "mapping.json")
            with open(mpath, "w", encoding="utf8") as f:   # the format clip/build_text_index.py writes and load_matrix reads
                for row in matrix:
                    f.write(" ".join("%.17g" % v for v in row) + "\n")   # 17 digits: the fp64 the reference reads IS the fp32 value
            with open(dpath, "w", encoding="utf8") as f:
                json.dump({str(i): c for i, c in enumerate(captions)}, f)
            u8 = make_images(ccfg.v_image, rng)
            index = ref_retrieval.CLIPIndex(mpath, dpath, clip)
            assert np.array_equal(index.load_matrix(mpath), matrix.astype(np.float64)), "the text file must hold the fp32 rows exactly"
            winners, rows, embeds = [], [], []
            for j in range(N_IMAGES):
                ipath = os.path.join(tmp, f"img{j}.png")
                Image.fromarray(u8[j]).save(ipath)
                winners.append(index.search_text(ipath))
                emb = clip.compute_batch_index_image_features([Image.open(ipath)]).numpy()
                embeds.append(emb[0])
                # the reference's own arithmetic (normalization, matmul against its fp64 index_matrix) on the fp64 image of the
                # embedding; its search_text normalises the fp32 embedding in fp32 first, which moves a score by ~1e-7
                rows.append(np.matmul(index.normalization(emb.astype(np.float64)), index.index_matrix.transpose())[0])
                fp32_path = np.matmul(index.get_image_representation(ipath), index.index_matrix.transpose())[0]
                assert np.abs(fp32_path - rows[-1]).max() < 1e-6 and fp32_path.argmax() == rows[-1].argmax()
            rows = np.stack(rows)
            top2 = np.sort(rows, axis=1)[:, -2:]
            if (top2[:, 1] - top2[:, 0] > MARGIN).all() and len(set(winners)) == N_IMAGES:
                break
        else:
            raise SystemExit("no seed gave every image its own winner with a margin above 1e-3")
    assert (top2[:, 1] - top2[:, 0] > MARGIN).all() and len(set(winners)) == N_IMAGES
    for j in range(N_IMAGES):
        assert captions[int(rows[j].argmax())] == winners[j]
    np.savez_compressed(os.path.join(HERE, "retrieval_tiny.npz"), index_matrix=matrix, images_u8=u8,
                        image_embeds=np.stack(embeds).astype(np.float32), scores=rows)
    with open(os.path.join(HERE, "retrieval_tiny.json"), "w", encoding="utf8") as f:
        json.dump(dict(seed=seed, mapping={str(i): c for i, c in enumerate(captions)}, winners=winners,
                       margins=[float(m) for m in top2[:, 1] - top2[:, 0]]), f, indent=1)
    print(f"[golden] retrieval_tiny: seed {seed}, {matrix.shape}, winners {[int(r.argmax()) for r in rows]}, "
          f"margins {[f'{m:.2e}' for m in top2[:, 1] - top2[:, 0]]}, "
          f"{os.path.getsize(os.path.join(HERE, 'retrieval_tiny.npz')) // 1024} KB")


if __name__ == "__main__":
    main()
