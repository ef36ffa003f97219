"""Drop-in for the reference's clip/clipretrieval.py `CLIPIndex` (the retrieval baseline): the same constructor and methods, the
search executed by the native engine (conzic_amd/retrieval.py::TextIndex -> czc_index_search).

    index = CLIPIndex(index_matrix_path, mapping_dict_path, clip)
    caption = index.search_text("image.jpg")
"""
from __future__ import annotations

import numpy as np

from conzic_amd.retrieval import TextIndex


class CLIPIndex:
    def __init__(self, index_matrix_path, mapping_dict_path, clip):
        self.index = TextIndex.load(index_matrix_path, mapping_dict_path)
        self.mapping_dict = {str(i): c for i, c in enumerate(self.index.captions)}
        self.clip = clip

    @staticmethod
    def normalization(matrix):
        matrix = np.asarray(matrix)
        return matrix / np.linalg.norm(matrix, axis=1, keepdims=True)

    @property
    def index_matrix(self):
        """The L2-normalised rows on the host, for callers that read the attribute; the search does not use it."""
        return self.normalization(self.index.matrix.astype(np.float64))

    def get_image_representation(self, image_path):
        from PIL import Image
        vec = self.clip.compute_batch_index_image_features([Image.open(image_path)])
        return self.normalization(np.asarray(vec, dtype=np.float32))

    def search_text(self, image_path):
        from PIL import Image
        (hits,) = self.index.search(self.clip, [Image.open(image_path)], 1)
        return hits[0][0]
