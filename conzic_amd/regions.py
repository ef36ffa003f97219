"""Regions of a picture for czc_preprocess_regions_u8 (include/conzic_hip.h): host-side boxes, the counterpart of rivals.py.

A region is a box (x0, y0, x1, y1) in PIL's crop convention -- pixel coordinates, x1 and y1 exclusive -- and stands for what
`PIL.Image.crop(box)` followed by the image processor produces.  This module parses, builds, checks and names boxes.  No GPU,
no engine.
"""
from __future__ import annotations

import json
from typing import List, Sequence, Tuple

MAX_REGIONS = 1024       # include/conzic_hip.h CZC_MAX_REGIONS
MAX_RESIZED = 1 << 24    # the largest resized long side int(S * long / short) the engine accepts

Box = Tuple[int, int, int, int]


def _box(values, what: str) -> Box:
    try:
        vals = list(values)
    except TypeError:
        raise ValueError(f"{what}: a box is x0,y0,x1,y1, got {values!r}") from None
    if len(vals) != 4:
        raise ValueError(f"{what}: a box is x0,y0,x1,y1, got {len(vals)} values")
    out = []
    for v in vals:
        if isinstance(v, bool) or (isinstance(v, float) and v != int(v)):
            raise ValueError(f"{what}: box coordinates are whole pixels, got {v!r}")
        try:
            out.append(int(v))
        except (TypeError, ValueError):
            raise ValueError(f"{what}: box coordinates are whole pixels, got {v!r}") from None
    return tuple(out)


def parse_boxes(text: str) -> List[Box]:
    """"x0,y0,x1,y1;x0,y0,x1,y1;..." -> [(x0, y0, x1, y1), ...] (empty pieces between ';' are skipped)."""
    boxes = []
    for piece in str(text).split(";"):
        if not piece.strip():
            continue
        fields = [f.strip() for f in piece.split(",")]
        if len(fields) != 4:
            raise ValueError(f"a box is x0,y0,x1,y1, got {piece.strip()!r}")
        try:
            boxes.append(tuple(int(f) for f in fields))
        except ValueError:
            raise ValueError(f"box coordinates are whole pixels, got {piece.strip()!r}") from None
    if not boxes:
        raise ValueError("no box given")
    return boxes


def grid_boxes(width: int, height: int, rows: int, cols: int) -> List[Box]:
    """rows x cols tiles, row by row: tile (r, c) = (c * width // cols, r * height // rows, (c + 1) * width // cols,
    (r + 1) * height // rows).  The tiles cover the image exactly and none is empty."""
    width, height, rows, cols = int(width), int(height), int(rows), int(cols)
    if width < 1 or height < 1:
        raise ValueError(f"grid_boxes: bad image size {width}x{height}")
    if rows < 1 or cols < 1:
        raise ValueError(f"grid_boxes: a grid needs at least one row and one column, got {rows}x{cols}")
    if rows > height or cols > width:
        raise ValueError(f"grid_boxes: a {rows}x{cols} grid has empty tiles on a {width}x{height} image")
    return [(c * width // cols, r * height // rows, (c + 1) * width // cols, (r + 1) * height // rows)
            for r in range(rows) for c in range(cols)]


def parse_grid(text: str) -> Tuple[int, int]:
    """"RxC" -> (rows, cols)."""
    parts = str(text).lower().split("x")
    try:
        rows, cols = (int(p) for p in parts)
    except ValueError:
        raise ValueError(f"a grid is ROWSxCOLS, e.g. 2x3, got {text!r}") from None
    if rows < 1 or cols < 1:
        raise ValueError(f"a grid needs at least one row and one column, got {text!r}")
    return rows, cols


def check_boxes(boxes: Sequence[Sequence[int]], width: int, height: int, size: int = 0) -> List[Box]:
    """The refusals of the C call, as ValueError with a readable message; returns the boxes as int tuples.  `size` (the
    processor's S; 0: not checked) adds the limit on the resized long side."""
    bx = [_box(b, f"box {i}") for i, b in enumerate(boxes)]
    if not 1 <= len(bx) <= MAX_REGIONS:
        raise ValueError(f"{len(bx)} regions: a call takes between 1 and {MAX_REGIONS}")
    for i, (x0, y0, x1, y1) in enumerate(bx):
        if x0 >= x1 or y0 >= y1:
            raise ValueError(f"box {i} = ({x0}, {y0}, {x1}, {y1}) is empty (x1 and y1 are exclusive)")
        if x0 < 0 or y0 < 0 or x1 > width or y1 > height:
            raise ValueError(f"box {i} = ({x0}, {y0}, {x1}, {y1}) leaves the {width}x{height} image "
                             "(PIL would pad with black; the engine refuses)")
        w, h = x1 - x0, y1 - y0
        if size and size * max(w, h) / min(w, h) > MAX_RESIZED:
            raise ValueError(f"box {i} = ({x0}, {y0}, {x1}, {y1}) resizes to a long side above 2^24")
    return bx


def region_name(name: str, box: Sequence[int]) -> str:
    """"name#x0,y0,x1,y1": the key of a region in logs, seeds and result files."""
    x0, y0, x1, y1 = _box(box, "region_name")
    return f"{name}#{x0},{y0},{x1},{y1}"


def load_regions_file(path: str) -> dict:
    """JSON {file name: [[x0, y0, x1, y1], ...]} -> {file name: [(x0, y0, x1, y1), ...]}."""
    with open(path, "r", encoding="utf-8") as f:
        raw = json.load(f)
    if not isinstance(raw, dict):
        raise ValueError(f"{path}: expected a JSON object {{file name: [[x0, y0, x1, y1], ...]}}")
    out = {}
    for name, boxes in raw.items():
        if not isinstance(boxes, list) or not boxes:
            raise ValueError(f"{path}: {name!r} needs a non-empty list of boxes")
        out[str(name)] = [_box(b, f"{path}: {name!r} box {i}") for i, b in enumerate(boxes)]
    return out
