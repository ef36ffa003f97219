#!/usr/bin/env python3
"""czc_generate with the step memo (option "memo") off and on, at the configs[2] shape (B = 256, K = 200, L = 15, sequential,
10 sweeps) on the converging setup of conzic_amd/harness.py::converging_setup (trained-like MLM head whose top words the CLIP
term picks among at the published logit scale: images reach a fixed point of the sweep at different sweeps, some not at all).
One engine, then one two-stream EngineGroup.

    python tools/memo_probe.py [--B 256] [--L 15] [--sweeps 10] [--alpha 0.02] [--reps 2] [--out profiles/r07_memo_probe.json]

Per run: captions/s both ways (best of --reps timed calls after one warm-up call), the hit fraction (czc_memo_stats), the
text-tower / BERT rows both ways (czc_stats), whether the ids of every sweep are identical, and how many image-steps hit
per sweep.  The JSON file holds one object per run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conzic_amd import harness, native  # noqa: E402
from conzic_amd.engine import EngineGroup  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=256)
ap.add_argument("--L", type=int, default=15)
ap.add_argument("--K", type=int, default=200)
ap.add_argument("--sweeps", type=int, default=10)
ap.add_argument("--alpha", type=float, default=0.02)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--streams", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_memo_probe.json"))
args = ap.parse_args()

su, emb, hp, init, seed_len = harness.converging_setup(B=args.B, L=args.L, precision=native.PREC_BF16, alpha=args.alpha)
eng = su.engine
pos = list(range(args.L)) * args.sweeps


def timed(runner, memo):
    runner.set_option("memo", memo)
    runner.generate(args.B, init, args.L, seed_len, args.K, pos, hp, snapshot_every=args.L)  # warm-up (workspace growth)
    best, res = 1e9, None
    for _ in range(args.reps):
        runner.profile_reset()
        t0 = time.perf_counter()
        ids, cos = runner.generate(args.B, init, args.L, seed_len, args.K, pos, hp, snapshot_every=args.L)
        dt = time.perf_counter() - t0
        if dt < best:
            best, res = dt, (ids, cos, runner.stats(), runner.memo_stats())
    return best, res


def probe(runner, label):
    t_off, (ids0, cos0, st0, _) = timed(runner, 0)
    t_on, (ids1, cos1, st1, ms) = timed(runner, 1)
    runner.set_option("memo", 0)
    hit_frac = ms["hit_image_steps"] / max(ms["image_steps"], 1)
    rec = dict(run=label, B=args.B, K=args.K, L=args.L, sweeps=args.sweeps, order="sequential", alpha=args.alpha, beta=2.0,
               logit_scale=4.6052, flat_top=8, precision="bf16", streams=(runner.streams if isinstance(runner, EngineGroup) else 1),
               captions_per_s_off=args.B / t_off, captions_per_s_on=args.B / t_on, speedup=t_off / t_on,
               wall_s_off=t_off, wall_s_on=t_on, hit_fraction=hit_frac, hit_image_steps=ms["hit_image_steps"],
               image_steps=ms["image_steps"], clip_rows_off=st0["clip_rows"], clip_rows_on=st1["clip_rows"],
               bert_rows_off=st0["bert_rows"], bert_rows_on=st1["bert_rows"], steps_run_off=st0["steps"],
               steps_run_on=st1["steps"], ids_identical=bool(np.array_equal(ids0, ids1)),
               cos_identical=bool(np.array_equal(cos0.view(np.int32), cos1.view(np.int32))),
               images_unchanged_per_sweep=[int((ids0[s] == ids0[s - 1]).all(axis=1).sum()) for s in range(1, ids0.shape[0])])
    if isinstance(runner, EngineGroup):
        rec["hit_fraction_per_stream"] = [e.memo_stats()["hit_image_steps"] / max(e.memo_stats()["image_steps"], 1)
                                          for e in runner.engines]
    print(json.dumps(rec), flush=True)
    return rec


recs = [probe(eng, "one engine")]
if args.streams > 1:
    grp = EngineGroup(eng, streams=args.streams, min_images=32)
    grp.set_image_embeds(emb)
    recs.append(probe(grp, f"EngineGroup, {args.streams} streams"))
    grp.close(parent=False)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(recs, f, indent=1)
eng.close()
