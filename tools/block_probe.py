#!/usr/bin/env python3
"""Block-synchronous sweeps of ONE caption: the serial sweep (runtime.run_generation, one position per step at batch size 1)
against runtime.run_generation_blocks at several block widths (czc_generate_rows_tied: `width` tied rows polish `width`
positions per step, ceil(L / width) steps per sweep).  One image, L = 10, K = 200, 10 sweeps, sequential order, interleaved
blocks, full-size synthetic towers, the bf16 and the screen-then-refine engine (logit scales 2.6592 and 4.6052).

    python tools/block_probe.py [--widths 1 2 5 10] [--reps 5] [--out profiles/r12_block_probe.json]

Per engine and width: the host wall time of the call, warm (one untimed call of every arm first), --reps repetitions alternated
between the arms, the median, the spread (max - min) / median, the ratio of width 1's median to the width's, and whether the
width was faster than width 1 in every repetition.  Width 1 is run_generation itself: the path without this feature.
On harness.converging_setup (a trained-like MLM head) it also records, per width, the cosine of the merged caption after the
last sweep (czc_score_rows) next to width 1's.  The random-weight towers say nothing about caption quality: that figure only
shows whether the block sweeps settle on captions the image term rates like the serial sweep's.

    python tools/block_probe.py --describe [profiles/r12_block_probe.json]

prints the README's sentence about that file (no GPU needed)."""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--widths", type=int, nargs="+", default=[1, 2, 5, 10])
ap.add_argument("--L", type=int, default=10)
ap.add_argument("--K", type=int, default=200)
ap.add_argument("--sweeps", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--scales", type=float, nargs="+", default=[2.6592, 4.6052])
ap.add_argument("--layout", default="interleaved", choices=["interleaved", "contiguous"])
ap.add_argument("--fluency", action="store_true",
                help="also record, per width, the merged caption's mean log p under BERT (Engine.fluency_rows) next to its cosine")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_block_probe.json"))
ap.add_argument("--describe", nargs="?", const=os.path.join(ROOT, "profiles", "r12_block_probe.json"), default=None, metavar="JSON",
                help="print the README sentence for a result file and exit")
args = ap.parse_args()
PROMPT = "Image of a"


def describe(path):
    parts = []
    for r in json.load(open(path)):
        ws = [w for w in r["widths"] if w["width"] != 1]
        base = next(w for w in r["widths"] if w["width"] == 1)
        said = ", ".join(f"width {w['width']} {w['wall_s_median']:.3f} s (x{w['ratio_to_width_1']:.2f}, spread {100 * w['spread']:.1f} %, "
                         + ("faster in every repetition" if w["faster_in_every_rep"] else
                            "slower in every repetition" if w["slower_in_every_rep"] else "the repetitions disagree in sign") + ")"
                         for w in ws)
        cos = ", ".join(f"{w['width']}: {w['converging_final_cos']:.4f}" for w in r["widths"])
        parts.append(f"on the {r['precision']} engine the serial sweep takes {base['wall_s_median']:.3f} s per caption of "
                     f"{r['sweeps']} sweeps (spread {100 * base['spread']:.1f} %); {said}; merged-caption cosine after the last sweep "
                     f"on the converging set-up by width {cos}")
    return "; ".join(parts)


if args.describe:
    print(describe(args.describe))
    sys.exit(0)

from conzic_amd import blocks, harness, native, runtime, synth  # noqa: E402
from conzic_amd.engine import Engine  # noqa: E402


def spread(ts):
    return (max(ts) - min(ts)) / float(np.median(ts))


def timing_leg(scale):
    from PIL import Image
    from clip.clip import CLIP
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab
    sv = harness.cached_vocab(False)
    bcfg, ccfg = synth.bert_base(), synth.clip_b32()
    ccfg.logit_scale = scale
    tok, clip_tok = tokenizers_from_vocab(sv)
    lm = SyntheticLM(bcfg)
    clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, 12), clip_tok)
    mask = synth.make_token_mask(sv, regular_only=True)
    image = Image.fromarray(synth.make_images_u8(1, ccfg.v_image)[0])
    logger = logging.getLogger("block_probe")
    logger.setLevel(logging.WARNING)
    names = ["img0"]

    def call(width):
        a = (names, lm, clip, tok, image, mask.copy(), PROMPT, logger, args.L, args.K, 0.1, 0.02, 2.0, args.sweeps, 1)
        if width == 1:   # the path without the feature
            return runtime.run_generation("sequential", *a, verbose=False)
        return runtime.run_generation_blocks("sequential", width, args.layout, 1, *a, verbose=False)[0]

    eng = runtime.get_engine(lm, clip, tok)
    finals = {w: call(w)[0][-2][0] for w in args.widths}   # warm-up of every arm
    times = {w: [] for w in args.widths}
    for _ in range(args.reps):
        for w in args.widths:
            eng.sync()
            t0 = time.perf_counter()
            call(w)
            times[w].append(time.perf_counter() - t0)
    prec = eng.precision
    runtime.evict()
    return prec, times, finals


def converging_leg(prec):
    su, _, hp, init, seed_len = harness.converging_setup(B=1, L=args.L, precision=prec)
    eng = su.engine
    out, flu = {}, {}
    try:
        for w in args.widths:
            if w == 1:
                pos, n_mask, every = harness.order_positions("sequential", args.L, args.sweeps)
                ids, _ = eng.generate(1, init, args.L, seed_len, args.K, pos, hp, n_mask=n_mask, snapshot_every=every)
                rows = ids[-1]
            else:
                one, nb = blocks.tied_positions([blocks.sequential_order(args.L, w, args.layout)] * args.sweeps, w)
                groups, _, ior = blocks.tied_rows(1, w)
                ids, _ = eng.generate_rows_tied(np.repeat(np.asarray(init, np.int32)[None, :], w, axis=0), None, seed_len, args.K, one,
                                                [hp] * w, None, groups, image_of_row=ior, snapshot_every=nb)
                rows = ids[-1, :1]
            out[w] = float(eng.score_rows(rows, seed_len)[0])   # one yardstick for every width: the caption as it stands
            if args.fluency:   # the other half of the objective: the same caption's mean log p under BERT
                flu[w] = float(eng.fluency_rows(rows, seed_len)["pll"][0]) / args.L
    finally:
        eng.close()
    return out, flu


def main():
    out = []
    for scale in args.scales:
        prec, times, finals = timing_leg(scale)
        cos, flu = converging_leg(prec)
        base = float(np.median(times[1])) if 1 in times else None
        rec = dict(logit_scale=scale, precision=runtime.PRECISION_NAMES[prec], L=args.L, K=args.K, sweeps=args.sweeps, order="sequential",
                   layout=args.layout, images=1, reps=args.reps, widths=[])
        for w in args.widths:
            med = float(np.median(times[w]))
            rec["widths"].append(dict(
                width=w, steps_per_sweep=blocks.n_blocks(args.L, w), wall_s=times[w], wall_s_median=med, spread=spread(times[w]),
                ratio_to_width_1=(base / med if base else None),
                faster_in_every_rep=bool(1 in times and w != 1 and all(t < t1 for t, t1 in zip(times[w], times[1]))),
                slower_in_every_rep=bool(1 in times and w != 1 and all(t > t1 for t, t1 in zip(times[w], times[1]))),
                final_caption=finals[w], converging_final_cos=cos[w]))
            if args.fluency:
                rec["widths"][-1]["converging_final_mean_logp"] = flu[w]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(describe(args.out))


if __name__ == "__main__":
    main()
