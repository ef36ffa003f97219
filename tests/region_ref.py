"""TEST INFRASTRUCTURE: the reference of a region -- PIL itself.  A region of an image is `Image.fromarray(im).crop(box)`
followed by the host statement of the image processor (oracle/imageproc.py); the boxes the GPU and CPU tests share."""
from __future__ import annotations

import numpy as np

from oracle.imageproc import preprocess

H, W = 97, 131   # the tiny engine's test image (S = 32)


def region_pixels(im: np.ndarray, boxes, S: int) -> np.ndarray:
    """fp32 [N, 3, S, S]: crop(box) in PIL, then the processor."""
    from PIL import Image
    pil = Image.fromarray(im)
    return preprocess([pil.crop(tuple(int(v) for v in b)) for b in boxes], S)


def slices(im: np.ndarray, boxes):
    """The contiguous copies im[y0:y1, x0:x1]."""
    return [np.ascontiguousarray(im[b[1]:b[3], b[0]:b[2]]) for b in boxes]


def make_image(h: int = H, w: int = W, seed: int = 3) -> np.ndarray:
    """Noise plus blocky structure, so that a misplaced window shows up as a large difference."""
    rng = np.random.default_rng(seed)
    im = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    im[: h // 2, : w // 3] //= 4
    return im


# (x0, y0, x1, y1) on the 97 x 131 (H x W) image, S = 32
BOXES = [
    (0, 0, W, H),            # full frame
    (40, 30, 72, 62),        # 32x32 interior: no pass runs
    (10, 5, 42, 92),         # 32 wide x 87 tall: the horizontal pass is skipped
    (7, 20, 124, 52),        # 117 wide x 32 tall: the vertical pass is skipped
    (0, 0, 1, 1),            # 1x1 at the top-left corner
    (W - 1, H - 1, W, H),    # 1x1 at the bottom-right corner
    (50, 0, 51, H),          # a 1 x 97 strip
    (0, 44, W, 45),          # a 131 x 1 strip
    (60, 40, 65, 47),        # 5x7: up-sampling
    (1, 2, 129, 95),         # 128x93: down-sampling with wide windows
    (0, 10, 20, 50),         # touches the left border
    (100, 0, W, 30),         # touches the top and the right border
    (30, 80, 90, H),         # touches the bottom border
    (110, 60, W, H),         # touches the right and the bottom border
    (20, 20, 70, 60),        # two identical boxes
    (20, 20, 70, 60),
    (40, 30, 100, 80),       # overlaps the two before it and the 32x32 one
]

# the full-size engine's case: a 480 x 640 (H x W) image, S = 224
H_FULL, W_FULL = 480, 640
BOXES_FULL = [
    (100, 100, 324, 324),    # 224x224 exact
    (50, 60, 450, 360),      # 400x300: down-sampling
    (300, 200, 350, 240),    # 50x40: up-sampling
    (600, 90, 610, 390),     # a 10 x 300 strip
    (0, 0, W_FULL, H_FULL),  # the full frame
    (500, 380, W_FULL, H_FULL),  # on the bottom-right corner
]
