"""Caption retrieval: a resident index of CLIP text embeddings on the engine (czc_index_set / czc_index_search,
include/conzic_hip.h) behind a small host class.

    index = TextIndex.from_captions(clip, captions)                  # or TextIndex.load(matrix_path, mapping_path)
    hits = index.search(clip, images, k=5)                           # per image: [(caption, cosine, id), ...]

The files are the reference's own (clip/build_text_index.py writes them, clip/clipretrieval.py::CLIPIndex reads them): the
matrix as text, one row of space-separated floats per line (`.npy` is accepted as well), and the mapping as JSON
{str(row): caption}.  The scan, the top-k and both normalisations run on the device; nothing here computes a score.
"""
from __future__ import annotations

import json
from typing import List, Sequence, Tuple

import numpy as np


class TextIndex:
    def __init__(self, matrix, captions: Sequence[str]):
        self.matrix = np.ascontiguousarray(np.asarray(matrix, dtype=np.float32))   # [N, D], un-normalised
        self.captions = [str(c) for c in captions]
        if self.matrix.ndim != 2 or self.matrix.shape[0] != len(self.captions):
            raise ValueError(f"TextIndex: {len(self.captions)} captions for a matrix of shape {self.matrix.shape}")
        if not len(self.captions):
            raise ValueError("TextIndex: no captions")

    def __len__(self):
        return len(self.captions)

    # ---- building / files ---------------------------------------------------------------------
    @classmethod
    def from_captions(cls, clip, captions: Sequence[str], chunk: int = 256) -> "TextIndex":
        """Encode `captions` with `clip.compute_text_representation`, `chunk` at a time."""
        captions = [str(c) for c in captions]
        if not captions:
            raise ValueError("TextIndex.from_captions: no captions")
        if chunk < 1:
            raise ValueError("TextIndex.from_captions: chunk must be >= 1")
        rows = [np.asarray(clip.compute_text_representation(captions[i:i + chunk]), dtype=np.float32)
                for i in range(0, len(captions), chunk)]
        return cls(np.concatenate(rows, axis=0), captions)

    @staticmethod
    def load_matrix(path: str) -> np.ndarray:
        if str(path).endswith(".npy"):
            return np.asarray(np.load(path), dtype=np.float32)
        rows = []
        with open(path, "r", encoding="utf8") as f:
            for line in f:
                vals = line.split()
                if vals:
                    rows.append(np.array(vals, dtype=np.float64))
        if not rows or len({r.size for r in rows}) != 1:
            raise ValueError(f"{path}: expected one row of space-separated floats per line, all of one length")
        return np.stack(rows).astype(np.float32)

    @classmethod
    def load(cls, index_matrix_path: str, mapping_dict_path: str) -> "TextIndex":
        matrix = cls.load_matrix(index_matrix_path)
        with open(mapping_dict_path, encoding="utf8") as f:
            mapping = json.load(f)
        missing = [i for i in range(matrix.shape[0]) if str(i) not in mapping]
        if missing or len(mapping) != matrix.shape[0]:
            raise ValueError(f"{mapping_dict_path}: {len(mapping)} captions for {matrix.shape[0]} index rows"
                             + (f" (row {missing[0]} has none)" if missing else ""))
        return cls(matrix, [mapping[str(i)] for i in range(matrix.shape[0])])

    def save(self, index_matrix_path: str, mapping_dict_path: str) -> None:
        if str(index_matrix_path).endswith(".npy"):
            np.save(index_matrix_path, self.matrix)
        else:
            with open(index_matrix_path, "w", encoding="utf8") as f:
                for row in self.matrix:
                    f.write(" ".join("%.9g" % v for v in row) + "\n")   # 9 digits: an fp32 value reads back as itself
        with open(mapping_dict_path, "w", encoding="utf8") as f:
            json.dump({str(i): c for i, c in enumerate(self.captions)}, f, indent=4)

    # ---- engine ---------------------------------------------------------------------------------
    def attach(self, engine) -> None:
        """Make this index the engine's (czc_index_set); a second call on the same engine does nothing."""
        if getattr(engine, "_text_index", None) is self and engine.index_size() == len(self):
            return
        if self.matrix.shape[1] != engine.clip_cfg.proj:
            raise ValueError(f"index rows have {self.matrix.shape[1]} dimensions, the engine's CLIP projects to {engine.clip_cfg.proj}")
        engine.index_set(self.matrix)
        engine._text_index = self

    def search_ids(self, clip, images, k: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """(ids int32 [B, k], cosines fp32 [B, k]) of `images` (PIL images / arrays, one or a list, or clip.ImageEmbeds), ordered by
        (cosine descending, id ascending); behind the index's last row the tail is (-1, -inf)."""
        emb = np.asarray(clip.compute_image_representation_from_image_instance(images), dtype=np.float32)
        engine = clip._eng()
        self.attach(engine)
        return engine.index_search(None, k, Q=int(emb.shape[0]))   # the embeddings the encode above left resident

    def search(self, clip, images, k: int = 1) -> List[List[Tuple[str, float, int]]]:
        """Per image the k nearest captions as (caption, cosine, id), best first."""
        ids, cos = self.search_ids(clip, images, k)
        return [[(self.captions[int(i)], float(c), int(i)) for i, c in zip(ids[b], cos[b]) if i >= 0] for b in range(ids.shape[0])]


def index_from_args(args, clip, logger=None) -> TextIndex:
    """The index of a `--run_type retrieve` run of the CLIs: loaded from --index_matrix_path / --mapping_dict_path, or built on
    the spot from the --index_captions file (one caption per line, empty lines skipped)."""
    if args.index_captions is not None:
        with open(args.index_captions, encoding="utf8") as f:
            captions = [line.strip() for line in f if line.strip()]
        if not captions:
            raise ValueError(f"--index_captions {args.index_captions}: no captions")
        index = TextIndex.from_captions(clip, captions)
    else:
        index = TextIndex.load(args.index_matrix_path, args.mapping_dict_path)
    if logger is not None:
        logger.info(f"text index: {len(index)} captions x {index.matrix.shape[1]} dimensions")
    return index
