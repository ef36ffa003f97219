"""Probe (no bound): N regions of one picture staged and encoded, the path without czc_preprocess_regions_u8 against the path
with it.

    python tools/regions_probe.py [--out profiles/r16_regions_probe.json]
    python tools/regions_probe.py --describe profiles/r16_regions_probe.json     # the README's sentence, from the file

Source: one 1280 x 960 synthetic picture, regions.grid_boxes at 4x4 and 8x8, full-size synthetic towers (bf16 engine).
Arm A, the path without the feature: N Engine.preprocess_u8 calls on host-cropped arrays (four small uploads and one
synchronisation each), then encode_staged(N).  Arm B: one Engine.preprocess_regions_u8 call, then encode_staged(N).  The host
clock runs around each arm, which ends in a device synchronise (encode_staged returns the embeddings); one warm-up per arm, then
--reps repetitions alternated between the arms; the record holds every time, each arm's median and spread ((max - min) / median),
the ratio of the medians, the same for the staging part alone (the arm without encode_staged, which also ends in a synchronise)
and whether both arms returned identical embeddings.  The ViT is in both arms; the staging-only figures say how much of an arm it
is."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--grids", default="4x4,8x8")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_regions_probe.json"))
ap.add_argument("--describe", default=None, metavar="JSON", help="print the README sentence for a result file and exit")
args = ap.parse_args()


def spread(ts):
    return float((max(ts) - min(ts)) / np.median(ts))


def describe(path):
    parts = []
    for r in json.load(open(path)):
        parts.append(f"{r['N']} regions ({r['grid']} tiles of a {r['width']}x{r['height']} picture): {r['wall_s_calls_median'] * 1e3:.1f} ms for "
                     f"{r['N']} preprocess_u8 calls on host crops + encode_staged (spread {100 * r['spread_calls']:.1f} %) against "
                     f"{r['wall_s_regions_median'] * 1e3:.1f} ms for one regions call + encode_staged (spread {100 * r['spread_regions']:.1f} %), "
                     f"ratio of the medians {r['ratio_median']:.2f}; staging alone {r['stage_s_calls_median'] * 1e3:.2f} ms against "
                     f"{r['stage_s_regions_median'] * 1e3:.2f} ms (ratio {r['stage_ratio_median']:.2f}), so the ViT is "
                     f"{100 * (1 - r['stage_s_regions_median'] / r['wall_s_regions_median']):.0f} % of the regions arm; embeddings "
                     f"{'identical' if r['identical'] else 'DIFFERENT'}")
    return "; ".join(parts)


if args.describe:
    print(describe(args.describe))
    sys.exit(0)

from conzic_amd import harness, native, regions  # noqa: E402

W, H = 1280, 960
rng = np.random.default_rng(16)
pic = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
pic[: H // 2, : W // 3] //= 4
su = harness.build_synthetic(False, native.PREC_BF16)
eng = su.engine
out = []
for grid in args.grids.split(","):
    rows, cols = regions.parse_grid(grid)
    boxes = regions.grid_boxes(W, H, rows, cols)
    N = len(boxes)
    crops = [np.ascontiguousarray(pic[y0:y1, x0:x1]) for x0, y0, x1, y1 in boxes]   # (host crops made outside the clock)

    def stage_calls():
        for i, c in enumerate(crops):
            eng.preprocess_u8(c, i)

    def stage_regions():
        eng.preprocess_regions_u8(pic, boxes, 0)

    arms = {"calls": stage_calls, "regions": stage_regions}
    emb = {}
    for arm, stage in arms.items():   # one warm-up per arm
        stage()
        emb[arm] = eng.encode_staged(N)
    wall = {a: [] for a in arms}
    stage_t = {a: [] for a in arms}
    for _ in range(args.reps):
        for arm, stage in arms.items():
            t0 = time.perf_counter()
            stage()
            e = eng.encode_staged(N)
            wall[arm].append(time.perf_counter() - t0)
            assert np.array_equal(e, emb[arm])
        for arm, stage in arms.items():
            t0 = time.perf_counter()
            stage()
            stage_t[arm].append(time.perf_counter() - t0)
    rec = dict(grid=grid, N=N, width=W, height=H, precision="bf16", reps=args.reps, identical=bool(np.array_equal(emb["calls"], emb["regions"])))
    for arm in arms:
        rec.update({f"wall_s_{arm}": wall[arm], f"wall_s_{arm}_median": float(np.median(wall[arm])), f"spread_{arm}": spread(wall[arm]),
                    f"stage_s_{arm}": stage_t[arm], f"stage_s_{arm}_median": float(np.median(stage_t[arm])),
                    f"stage_spread_{arm}": spread(stage_t[arm])})
    rec["ratio_median"] = rec["wall_s_calls_median"] / rec["wall_s_regions_median"]
    rec["stage_ratio_median"] = rec["stage_s_calls_median"] / rec["stage_s_regions_median"]
    out.append(rec)
    print(json.dumps(rec), flush=True)
    assert rec["identical"], "the two arms returned different embeddings"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(describe(args.out))
eng.close()
