#!/usr/bin/env python3
"""S samples of ONE image: the serial sample loop (S czc_generate calls at batch size 1, what demo.py:83 does) against one
czc_generate_rows call with S rows, every sample under its own shuffle order.  Full-size towers, L = 10, K = 200, 10 sweeps,
the precision the runtime picks for the logit scale (2.6592 -> bf16, 4.6052 -> screen-then-refine).

    python tools/rows_probe.py [--S 1 2 4 8 16] [--reps 3] [--out profiles/r08_rows_probe.json]

Per (logit scale, S): wall time of both arms, warm (one untimed call of each first), --reps repetitions alternating
serial / rows, whether the ids of every sweep agree row for row, and the ratios.  The JSON file holds one object per case.

    python tools/rows_probe.py --memo_rows [--S 4 16] [--reps 5] [--off_only] [--out profiles/r09_memo_rows_probe.json]

The rows call with the per-row step memo (option "memo_rows") off and on, on the converging set-up (harness.converging_setup:
a trained-like MLM head, rows settle after a few sweeps), one image x S rows, bf16 and screen-then-refine engines.  Per (engine,
S): wall times of --reps alternating off / on calls after one warm-up of each, their spread ((max - min) / median), the hit
fraction (czc_memo_rows_stats) and whether ids and cosines agree.  --off_only never touches the option: the option-off arm
alone, e.g. on a library built from another commit (CZC_LIB_PATH) for an A/B of the unchanged path.

    python tools/rows_probe.py --lengths 6,8,10,12 [--reps 5] [--out profiles/r09_lengths_probe.json]

One image at several sentence lengths: the serial loop (one czc_generate call at batch size 1 per length) against one
czc_generate_rows_len call with one row per length, every row under its own shuffle order (lengths.length_schedules).  Full-size
towers, both logit scales; per scale the wall times of --reps alternating serial / one-call repetitions after one warm-up of
each, their spread, whether the one call was faster in every repetition and whether every sweep's ids agree row for row.

    python tools/rows_probe.py --sample_tau 0.5 [--S 16] [--reps 5] [--out profiles/r11_draw_probe.json]

The cost of sampled winners: one image x S rows under their own shuffle orders, one czc_generate_rows_draw call with every tau 0
(the argmax path, i.e. czc_generate_rows_hp) against the same call with every tau = --sample_tau and a seed per row.  Full-size
towers, both logit scales; per scale the wall times of --reps alternating repetitions after one warm-up of each, each arm's spread
((max - min) / median), the median ratio, and the distinct final captions and Div-1 / Div-2 (over token ids) of each arm.
`--describe_draw profiles/r11_draw_probe.json` prints the README's sentence about that file (no GPU needed).

    python tools/rows_probe.py --distinct 1.0 [--S 16] [--reps 5] [--out profiles/r13_rival_probe.json]

The cost of rival images: 8 resident images x S rows under their own shuffle orders, one czc_generate_rows_vs call with
rival_of_row = NULL (czc_generate_rows_tied itself: the path without the feature) against the same call with the 4 nearest other
images as every row's rivals and delta = --distinct.  Full-size towers, both logit scales (the screen-then-refine engine refuses
rivals, so the published scale runs on the split-fp16 engine, where the runtime sends such a call); per scale the wall times of
--reps alternating repetitions after one warm-up of each arm, each arm's spread, the ratio of the medians and the share of final
captions the term changed.  `--describe_distinct profiles/r13_rival_probe.json` prints the README's sentence (no GPU needed).

    python tools/rows_probe.py --vocab [--S 16] [--reps 5] [--out profiles/r15_vocab_probe.json]

The cost of vocabulary sets: S rows of one image under their own shuffle orders, one czc_generate_rows_vocab call with
set_of_row = NULL (czc_generate_rows_vs itself, the path without the feature) against the same call in which every row carries a
ban-list of 100 regular ids.  Full-size towers, both logit scales; arms alternated, one warm-up each.  Records per arm the wall
times, their median and spread, the median ratio, and whether the set arm's ids are those of the NULL arm under a token mask with
the 100 ids taken out by hand (property E).  `--describe_vocab profiles/r15_vocab_probe.json` prints the README's sentence (no GPU
needed)."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conzic_amd import harness, runtime  # noqa: E402
from conzic_amd.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--S", type=int, nargs="+", default=[1, 2, 4, 8, 16])
ap.add_argument("--L", type=int, default=10)
ap.add_argument("--K", type=int, default=200)
ap.add_argument("--sweeps", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--scales", type=float, nargs="+", default=[2.6592, 4.6052])
ap.add_argument("--out", default=None)
ap.add_argument("--memo_rows", action="store_true", help="the memo_rows leg instead of the serial / rows comparison")
ap.add_argument("--off_only", action="store_true", help="--memo_rows: time the option-off arm only and leave the option alone")
ap.add_argument("--lengths", type=lambda v: [int(n) for n in v.split(",")], default=None, metavar="L1,L2,...",
                help="the lengths leg: one call per length against one czc_generate_rows_len call")
ap.add_argument("--signals", default=None, metavar="caption,positive,negative",
                help="the signals leg: one call per control signal against one czc_generate_rows_hp call (table mode)")
ap.add_argument("--sample_tau", type=float, default=None, metavar="T",
                help="the draw leg: the rows call with every tau = 0 against the same call with every tau = T")
ap.add_argument("--distinct", type=float, default=None, metavar="DELTA",
                help="the rivals leg: the rows call with rival_of_row = NULL against the same call with 4 rivals per row")
ap.add_argument("--vocab", action="store_true", help="the vocabulary-set leg: set_of_row = NULL against a ban-list of 100 ids in every row")
ap.add_argument("--describe_vocab", default=None, metavar="JSON", help="print the README sentence for a vocabulary-leg result file and exit")
ap.add_argument("--fluency_probe", action="store_true",
                help="the fluency leg: Engine.fluency_rows on R captions of L words against the path without it (L steps that return "
                     "their logits row + a host log-softmax); R from --S")
ap.add_argument("--describe_fluency", default=None, metavar="JSON", help="print the README sentence for a fluency-leg result file and exit")
ap.add_argument("--describe_distinct", default=None, metavar="JSON", help="print the README sentence for a rivals-leg result file and exit")
ap.add_argument("--describe_draw", default=None, metavar="JSON", help="print the README sentence for a draw-leg result file and exit")
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "r15_vocab_probe.json" if args.vocab else "r14_fluency_probe.json" if args.fluency_probe else "r13_rival_probe.json" if args.distinct else "r11_draw_probe.json" if args.sample_tau else "r10_signals_probe.json" if args.signals else "r09_lengths_probe.json" if args.lengths else
                            "r09_memo_rows_probe.json" if args.memo_rows else "r08_rows_probe.json")

L, K, SEED_LEN = args.L, args.K, 4
out = []


def describe_draw(path):
    """The README's sentence, from the file: a ratio inside the argmax arm's own spread is "no measurable cost"."""
    parts = []
    for r in json.load(open(path)):
        inside = abs(r["ratio_median"] - 1.0) <= r["spread_argmax"]
        verdict = "no measurable cost" if inside else (f"x{r['ratio_median']:.3f} the argmax arm" + (
            "; its steps are never margin-gated, so it re-encodes %d candidate sequences against %d" % (r["refine_seqs_draw"], r["refine_seqs_argmax"])
            if r["precision"] == "refine" else ""))
        parts.append(f"on the {r['precision']} engine {r['wall_s_argmax_median']:.3f} s with every tau = 0 (spread {100 * r['spread_argmax']:.1f} %) and "
                     f"{r['wall_s_draw_median']:.3f} s with tau = {r['tau']:g} (spread {100 * r['spread_draw']:.1f} %), ratio of the medians "
                     f"{r['ratio_median']:.3f}: {verdict}; {r['distinct_captions_argmax']} -> {r['distinct_captions_draw']} distinct captions of "
                     f"{r['S']}, Div-1 {r['div1_ids_argmax']:.2f} -> {r['div1_ids_draw']:.2f} and Div-2 {r['div2_ids_argmax']:.2f} -> "
                     f"{r['div2_ids_draw']:.2f} over token ids")
    return "; ".join(parts)


if args.describe_draw:
    print(describe_draw(args.describe_draw))
    sys.exit(0)


def describe_distinct(records):
    """The README's sentence, from the records of a result file: a ratio inside the NULL arm's own spread is "no measurable cost"."""
    parts = []
    for r in records:
        inside = abs(r["ratio_median"] - 1.0) <= r["spread_null"]
        parts.append(f"on the {r['precision']} engine {r['wall_s_null_median']:.3f} s with rival_of_row = NULL (spread {100 * r['spread_null']:.1f} %) "
                     f"and {r['wall_s_rivals_median']:.3f} s with {r['M']} rivals per row and delta = {r['delta']:g} (spread "
                     f"{100 * r['spread_rivals']:.1f} %), ratio of the medians {r['ratio_median']:.3f}: "
                     + ("no measurable cost" if inside else f"x{r['ratio_median']:.3f} the NULL arm")
                     + f"; the term changed {r['captions_changed']} of {r['S']} final captions")
    return "; ".join(parts)


if args.describe_distinct:
    print(describe_distinct(json.load(open(args.describe_distinct))))
    sys.exit(0)


def describe_vocab(records):
    """The README's sentence, from the records of a result file: a ratio inside the NULL arm's own spread is "no measurable cost"."""
    parts = []
    for r in records:
        inside = abs(r["ratio_median"] - 1.0) <= r["spread_null"]
        parts.append(f"on the {r['precision']} engine {r['wall_s_null_median']:.3f} s with set_of_row = NULL (spread {100 * r['spread_null']:.1f} %) "
                     f"and {r['wall_s_sets_median']:.3f} s with a ban-list of {r['banned']} ids in every row (spread "
                     f"{100 * r['spread_sets']:.1f} %), ratio of the medians {r['ratio_median']:.3f}: "
                     + ("no measurable cost" if inside else f"x{r['ratio_median']:.3f} the NULL arm")
                     + f"; the ids are {'' if r['ids_identical_to_E'] else 'NOT '}those of the call without sets under the token mask with "
                       f"the ids taken out by hand, and the list changed {r['captions_changed']} of {r['S']} final captions")
    return "; ".join(parts)


if args.describe_vocab:
    print(describe_vocab(json.load(open(args.describe_vocab))))
    sys.exit(0)


def spread(ts):
    return (max(ts) - min(ts)) / float(np.median(ts))


def describe_fluency(records):
    """The README's sentence, from the records of a result file."""
    return "; ".join(f"on the {r['precision']} engine, R = {r['R']} captions of L = {r['L']}: {r['wall_s_fluency_median'] * 1e3:.1f} ms for "
                     f"fluency_rows (spread {100 * r['spread_fluency']:.1f} %) against {r['wall_s_steps_median'] * 1e3:.1f} ms for {r['L']} steps "
                     f"that return their logits row plus the host log-softmax (spread {100 * r['spread_steps']:.1f} %), ratio of the medians "
                     f"{r['ratio_median']:.2f}; largest |log p| difference between the two {r['max_abs_diff']:.1e}" for r in records)


if args.describe_fluency:
    print(describe_fluency(json.load(open(args.describe_fluency))))
    sys.exit(0)


def fluency_leg():
    """Full-size synthetic towers, arms alternated, median of 5: one fluency_rows call against what a user does without it."""
    reps = max(args.reps, 5)
    for scale in args.scales:
        prec = runtime.choose_precision(scale)
        su = harness.build_synthetic(False, prec, logit_scale=scale, regular_only=True)
        eng = su.engine
        regular = np.nonzero(su.token_mask[0] > 0)[0]
        for R in (args.S if args.S != [1, 2, 4, 8, 16] else [16]):
            rows = np.repeat(np.asarray(su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L), np.int32)[None, :], R, axis=0)
            rows[:, SEED_LEN:SEED_LEN + L] = np.random.default_rng(5).choice(regular, size=(R, L))
            eng.set_image_embeds(np.random.default_rng(100).standard_normal((R, su.clip_cfg.proj)).astype(np.float32))
            hp = Engine.hyper(0.02, 2.0, 1.0)

            def fluency():
                return eng.fluency_rows(rows, SEED_LEN)["logp"]

            def steps():   # every step also runs a CLIP tower nobody wants: that is the path as it stands
                logp = np.empty((R, L), np.float32)
                for j in range(L):
                    x = eng.step(rows.copy(), SEED_LEN + j, K, hp, want=("logits",))["logits"].astype(np.float64)
                    lse = x.max(axis=1) + np.log(np.exp(x - x.max(axis=1, keepdims=True)).sum(axis=1))
                    logp[:, j] = x[np.arange(R), rows[:, SEED_LEN + j]] - lse
                return logp

            arms = {"fluency": fluency, "steps": steps}
            warm = {arm: fn() for arm, fn in arms.items()}
            times = {arm: [] for arm in arms}
            for _ in range(reps):
                for arm, fn in arms.items():
                    eng.sync()
                    t0 = time.perf_counter()
                    fn()
                    times[arm].append(time.perf_counter() - t0)
            rec = dict(logit_scale=scale, precision=runtime.PRECISION_NAMES[prec], R=R, L=L, K=K, reps=reps,
                       max_abs_diff=float(np.abs(warm["fluency"] - warm["steps"]).max()))
            for arm in arms:
                rec.update({f"wall_s_{arm}": times[arm], f"wall_s_{arm}_median": float(np.median(times[arm])), f"spread_{arm}": spread(times[arm])})
            rec["ratio_median"] = rec["wall_s_steps_median"] / rec["wall_s_fluency_median"]
            print(json.dumps(rec), flush=True)
            out.append(rec)
        eng.close()
    print(describe_fluency(out))


def memo_rows_leg():
    from conzic_amd import native
    for prec in (native.PREC_BF16, native.PREC_REFINE):
        su, _, hp, init, seed_len = harness.converging_setup(B=1, L=L, precision=prec)
        eng = su.engine
        for S in (args.S if args.S != [1, 2, 4, 8, 16] else [4, 16]):
            random.seed(42)
            positions, n_mask, every, _ = harness.sample_schedules("shuffle", L, args.sweeps, S)
            arms = (0,) if args.off_only else (0, 1)

            def call(on):
                if not args.off_only:
                    eng.set_option("memo_rows", on)
                eng.profile_reset()
                res = eng.generate_rows(init, L, seed_len, K, positions, hp, image_of_row=[0] * S, n_mask=n_mask, snapshot_every=every)
                return res, (None if args.off_only else eng.memo_rows_stats())

            warm = {on: call(on) for on in arms}
            times = {on: [] for on in arms}
            for _ in range(args.reps):
                for on in arms:
                    eng.sync()
                    t0 = time.perf_counter()
                    call(on)
                    times[on].append(time.perf_counter() - t0)
            rec = dict(precision=runtime.PRECISION_NAMES[prec], S=S, L=L, K=K, sweeps=args.sweeps, order="shuffle", images=1,
                       wall_s_off=times[0], wall_s_off_median=float(np.median(times[0])), spread_off=spread(times[0]))
            if not args.off_only:
                ms = warm[1][1]
                rec.update(wall_s_on=times[1], wall_s_on_median=float(np.median(times[1])), spread_on=spread(times[1]),
                           speedup_median=float(np.median(times[0]) / np.median(times[1])),
                           hit_fraction=ms["hit_row_steps"] / max(ms["row_steps"], 1),
                           ids_identical=bool(np.array_equal(warm[0][0][0], warm[1][0][0])),
                           cos_max_abs_diff=float(np.abs(warm[0][0][1] - warm[1][0][1]).max()))
            print(json.dumps(rec), flush=True)
            out.append(rec)
        eng.close()


def lengths_leg():
    from conzic_amd import lengths
    lens = args.lengths
    for scale in args.scales:
        prec = runtime.choose_precision(scale)
        su = harness.build_synthetic(False, prec, logit_scale=scale, regular_only=True)
        eng = su.engine
        eng.set_image_embeds(np.random.default_rng(100).standard_normal((1, su.clip_cfg.proj)).astype(np.float32))
        hp = Engine.hyper(0.02, 2.0, 0.1)
        init = lengths.length_rows(su.bert_tok, "Image of a", lens)
        random.seed(42)
        positions, n_mask, every = lengths.length_schedules(lens, "shuffle", args.sweeps)
        own = [positions.reshape(args.sweeps, every, len(lens))[:, :n, r].reshape(-1).tolist() for r, n in enumerate(lens)]

        def serial():
            return [eng.generate(1, init[r, :SEED_LEN + n + 1].tolist(), n, SEED_LEN, K, own[r], hp, snapshot_every=n)
                    for r, n in enumerate(lens)]

        def one_call():
            return eng.generate_rows_len(init, lens, SEED_LEN, K, positions, hp, image_of_row=[0] * len(lens), n_mask=n_mask,
                                         snapshot_every=every)

        ref, got = serial(), one_call()  # warm-up (workspace growth) and the comparison
        same = all(np.array_equal(ref[r][0][:, 0], got[0][:, r, :SEED_LEN + n + 1]) for r, n in enumerate(lens))
        cos_diff = max(float(np.abs(ref[r][1][:, 0] - got[1][:, r]).max()) for r in range(len(lens)))
        t_serial, t_one = [], []
        for _ in range(args.reps):
            for fn, acc in ((serial, t_serial), (one_call, t_one)):
                eng.sync()
                t0 = time.perf_counter()
                fn()
                acc.append(time.perf_counter() - t0)
        rec = dict(logit_scale=scale, precision=runtime.PRECISION_NAMES[prec], lengths=lens, K=K, sweeps=args.sweeps, order="shuffle",
                   images=1, wall_s_serial=t_serial, wall_s_one_call=t_one, spread_serial=spread(t_serial), spread_one_call=spread(t_one),
                   speedup_median=float(np.median(t_serial) / np.median(t_one)),
                   speedup_min=min(a / b for a, b in zip(t_serial, t_one)), speedup_max=max(a / b for a, b in zip(t_serial, t_one)),
                   one_call_faster_in_every_rep=all(b < a for a, b in zip(t_serial, t_one)), ids_identical=bool(same),
                   cos_max_abs_diff=cos_diff)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        eng.close()


def signals_leg():
    """One image, every signal a row of L positions under its own run's order: one scalar call per signal (the serial arm)
    against one czc_generate_rows_hp call, synthetic control tables, alternating repetitions."""
    from conzic_amd import signals as sg, synth
    sigs = sg.parse_signals(args.signals)
    for scale in args.scales:
        prec = runtime.choose_precision(scale)
        su = harness.build_synthetic(False, prec, logit_scale=scale, regular_only=True, lexicon=True)
        eng = su.engine
        V = len(su.sv.bert_tokens)
        eng.set_pos(synth.make_pos_tags(V), synth.pos_template_masks([["DET"], ["ADJ", "NOUN"], ["NOUN"], ["VERB"]]))
        eng.set_image_embeds(np.random.default_rng(100).standard_normal((1, su.clip_cfg.proj)).astype(np.float32))
        random.seed(42)
        rows = sg.expand(sigs, [L], 1, "shuffle", args.sweeps, alpha=0.02, beta=2.0, temperature=0.1, gamma=5.0)
        init, row_lens, positions, hypers, ior = sg.batch_rows(rows, su.bert_tok, "Image of a", 1)

        def serial():
            return [eng.generate(1, init[c].tolist(), L, SEED_LEN, K, positions[:, c].tolist(), hypers[c], n_mask=rows.n_mask,
                                 snapshot_every=rows.every) for c in range(len(sigs))]

        def one_call():
            return eng.generate_rows_hp(init, row_lens, SEED_LEN, K, positions, hypers, image_of_row=ior, n_mask=rows.n_mask,
                                        snapshot_every=rows.every)

        ref, got = serial(), one_call()  # warm-up (workspace growth) and the comparison
        same = all(np.array_equal(ref[c][0][:, 0], got[0][:, c]) for c in range(len(sigs)))
        cos_diff = max(float(np.abs(ref[c][1][:, 0] - got[1][:, c]).max()) for c in range(len(sigs)))
        t_serial, t_one = [], []
        for _ in range(args.reps):
            for fn, acc in ((serial, t_serial), (one_call, t_one)):
                eng.sync()
                t0 = time.perf_counter()
                fn()
                acc.append(time.perf_counter() - t0)
        rec = dict(logit_scale=scale, precision=runtime.PRECISION_NAMES[prec], signals=sigs, L=L, K=K, sweeps=args.sweeps, order="shuffle",
                   images=1, wall_s_serial=t_serial, wall_s_one_call=t_one, spread_serial=spread(t_serial), spread_one_call=spread(t_one),
                   speedup_median=float(np.median(t_serial) / np.median(t_one)),
                   speedup_min=min(a / b for a, b in zip(t_serial, t_one)), speedup_max=max(a / b for a, b in zip(t_serial, t_one)),
                   one_call_faster_in_every_rep=all(b < a for a, b in zip(t_serial, t_one)), ids_identical=bool(same),
                   cos_max_abs_diff=cos_diff)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        eng.close()


def draw_leg():
    from conzic_amd import draws as dw, lengths
    tau = float(args.sample_tau)
    for scale in args.scales:
        prec = runtime.choose_precision(scale)
        su = harness.build_synthetic(False, prec, logit_scale=scale, regular_only=True)
        eng = su.engine
        eng.set_image_embeds(np.random.default_rng(100).standard_normal((1, su.clip_cfg.proj)).astype(np.float32))
        for S in (args.S if args.S != [1, 2, 4, 8, 16] else [16]):
            init = lengths.length_rows(su.bert_tok, "Image of a", [L] * S)
            hps = [Engine.hyper(0.02, 2.0, 0.1) for _ in range(S)]
            random.seed(42)
            positions, n_mask, every, _ = harness.sample_schedules("shuffle", L, args.sweeps, S)
            seeds = [dw.row_seed(42, 0, s) for s in range(S)]
            arms = {"argmax": dw.draw_rows(seeds, 0.0), "draw": dw.draw_rows(seeds, tau)}

            def call(arm):
                eng.profile_reset()
                res = eng.generate_rows_draw(init, None, SEED_LEN, K, positions, hps, arms[arm], image_of_row=[0] * S, n_mask=n_mask,
                                             snapshot_every=every)
                return res, eng.stats()

            warm = {arm: call(arm) for arm in arms}
            times = {arm: [] for arm in arms}
            for _ in range(args.reps):
                for arm in arms:
                    eng.sync()
                    t0 = time.perf_counter()
                    call(arm)
                    times[arm].append(time.perf_counter() - t0)
            rec = dict(logit_scale=scale, precision=runtime.PRECISION_NAMES[prec], S=S, L=L, K=K, sweeps=args.sweeps, order="shuffle",
                       images=1, tau=tau)
            for arm in arms:
                finals = warm[arm][0][0][-1][:, SEED_LEN:SEED_LEN + L]
                grams = {n: [tuple(r[i:i + n]) for r in finals.tolist() for i in range(L - n + 1)] for n in (1, 2)}
                rec.update({f"wall_s_{arm}": times[arm], f"wall_s_{arm}_median": float(np.median(times[arm])),
                            f"spread_{arm}": spread(times[arm]), f"distinct_captions_{arm}": len({r.tobytes() for r in finals}),
                            f"div1_ids_{arm}": len(set(grams[1])) / len(grams[1]), f"div2_ids_{arm}": len(set(grams[2])) / len(grams[2]),
                            f"refine_seqs_{arm}": warm[arm][1]["refine_seqs"], f"gated_image_steps_{arm}": warm[arm][1]["gated_image_steps"]})
            rec["ratio_median"] = rec["wall_s_draw_median"] / rec["wall_s_argmax_median"]
            rec["ratio_inside_argmax_spread"] = bool(abs(rec["ratio_median"] - 1.0) <= rec["spread_argmax"])
            print(json.dumps(rec), flush=True)
            out.append(rec)
        eng.close()


def distinct_leg():
    from conzic_amd import lengths, native, rivals as rv
    n_img, M = 8, 4
    for scale in args.scales:
        prec = runtime.choose_precision(scale)
        if prec == native.PREC_REFINE:   # czc_generate_rows_vs refuses it; the runtime sends such a call to the split engine
            prec = native.PREC_SPLIT
        su = harness.build_synthetic(False, prec, logit_scale=scale, regular_only=True)
        eng = su.engine
        emb = np.random.default_rng(100).standard_normal((n_img, su.clip_cfg.proj)).astype(np.float32)
        eng.set_image_embeds(emb)
        for S in (args.S if args.S != [1, 2, 4, 8, 16] else [16]):
            init = lengths.length_rows(su.bert_tok, "Image of a", [L] * S)
            hps = [Engine.hyper(0.02, 2.0, 0.1) for _ in range(S)]
            random.seed(42)
            positions, n_mask, every, _ = harness.sample_schedules("shuffle", L, args.sweeps, S)
            ior = np.arange(S, dtype=np.int32) % n_img
            arms = {"null": None, "rivals": rv.expand(rv.rival_table(emb, M), ior)}
            deltas = np.full(S, float(args.distinct), np.float32)

            def call(arm):
                return eng.generate_rows_vs(init, None, SEED_LEN, K, positions, hps, None, None, arms[arm], deltas, image_of_row=ior,
                                            n_mask=n_mask, snapshot_every=every)

            warm = {arm: call(arm) for arm in arms}
            times = {arm: [] for arm in arms}
            for _ in range(args.reps):
                for arm in arms:
                    eng.sync()
                    t0 = time.perf_counter()
                    call(arm)
                    times[arm].append(time.perf_counter() - t0)
            rec = dict(logit_scale=scale, precision=runtime.PRECISION_NAMES[prec], S=S, L=L, K=K, sweeps=args.sweeps, order="shuffle",
                       images=n_img, M=M, delta=float(args.distinct))
            for arm in arms:
                rec.update({f"wall_s_{arm}": times[arm], f"wall_s_{arm}_median": float(np.median(times[arm])),
                            f"spread_{arm}": spread(times[arm])})
            rec["ratio_median"] = rec["wall_s_rivals_median"] / rec["wall_s_null_median"]
            rec["ratio_inside_null_spread"] = bool(abs(rec["ratio_median"] - 1.0) <= rec["spread_null"])
            rec["captions_changed"] = int((warm["null"][0][-1] != warm["rivals"][0][-1]).any(axis=1).sum())
            print(json.dumps(rec), flush=True)
            out.append(rec)
        eng.close()
    print(describe_distinct(out))


def vocab_leg():
    from conzic_amd import lengths, vocab as vc
    reps = max(args.reps, 5)
    for scale in args.scales:
        prec = runtime.choose_precision(scale)
        su = harness.build_synthetic(False, prec, logit_scale=scale, regular_only=True)
        eng = su.engine
        eng.set_image_embeds(np.random.default_rng(100).standard_normal((1, su.clip_cfg.proj)).astype(np.float32))
        mask = su.token_mask.reshape(-1).astype(np.float32)
        banned = np.random.default_rng(7).choice(np.nonzero(mask > 0)[0], size=100, replace=False)
        allowed = np.ones(mask.size, bool)
        allowed[banned] = False
        bits = vc.pack([allowed], mask.size)
        for S in (args.S if args.S != [1, 2, 4, 8, 16] else [16]):
            init = lengths.length_rows(su.bert_tok, "Image of a", [L] * S)
            hps = [Engine.hyper(0.02, 2.0, 0.1) for _ in range(S)]
            random.seed(42)
            positions, n_mask, every, _ = harness.sample_schedules("shuffle", L, args.sweeps, S)
            ior = np.zeros(S, dtype=np.int32)
            arms = {"null": None, "sets": np.zeros(S, np.int32)}

            def call(arm):
                return eng.generate_rows_vocab(init, None, SEED_LEN, K, positions, hps, sets=bits, set_of_row=arms[arm], image_of_row=ior,
                                               n_mask=n_mask, snapshot_every=every)

            warm = {arm: call(arm) for arm in arms}
            eng.set_token_mask(mask * allowed)   # property E: the NULL arm under the mask with the ids taken out by hand
            by_hand = call("null")
            eng.set_token_mask(mask)
            times = {arm: [] for arm in arms}
            for _ in range(reps):
                for arm in arms:
                    eng.sync()
                    t0 = time.perf_counter()
                    call(arm)
                    times[arm].append(time.perf_counter() - t0)
            rec = dict(logit_scale=scale, precision=runtime.PRECISION_NAMES[prec], S=S, L=L, K=K, sweeps=args.sweeps, order="shuffle",
                       images=1, banned=int(banned.size), reps=reps)
            for arm in arms:
                rec.update({f"wall_s_{arm}": times[arm], f"wall_s_{arm}_median": float(np.median(times[arm])),
                            f"spread_{arm}": spread(times[arm])})
            rec["ratio_median"] = rec["wall_s_sets_median"] / rec["wall_s_null_median"]
            rec["ratio_inside_null_spread"] = bool(abs(rec["ratio_median"] - 1.0) <= rec["spread_null"])
            rec["ids_identical_to_E"] = bool(np.array_equal(warm["sets"][0], by_hand[0]))
            rec["cos_bits_identical_to_E"] = bool(np.array_equal(warm["sets"][1].view(np.int32), by_hand[1].view(np.int32)))
            rec["captions_changed"] = int((warm["null"][0][-1] != warm["sets"][0][-1]).any(axis=1).sum())
            print(json.dumps(rec), flush=True)
            out.append(rec)
        eng.close()
    print(describe_vocab(out))


if args.vocab:
    vocab_leg()
elif args.fluency_probe:
    fluency_leg()
elif args.distinct:
    distinct_leg()
elif args.sample_tau:
    draw_leg()
elif args.memo_rows:
    memo_rows_leg()
elif args.signals:
    signals_leg()
elif args.lengths:
    lengths_leg()
for scale in ([] if args.vocab or args.fluency_probe or args.memo_rows or args.lengths or args.signals or args.sample_tau or args.distinct else args.scales):
    prec = runtime.choose_precision(scale)
    su = harness.build_synthetic(False, prec, logit_scale=scale, regular_only=True)
    eng = su.engine
    emb = np.random.default_rng(100).standard_normal((1, su.clip_cfg.proj)).astype(np.float32)
    eng.set_image_embeds(emb)
    init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)
    hp = Engine.hyper(0.02, 2.0, 0.1)
    for S in args.S:
        random.seed(42)
        positions, n_mask, every, _ = harness.sample_schedules("shuffle", L, args.sweeps, S)

        def serial():
            return [eng.generate(1, init, L, SEED_LEN, K, positions[:, s].tolist(), hp, n_mask=n_mask, snapshot_every=every)
                    for s in range(S)]

        def rows():
            return eng.generate_rows(init, L, SEED_LEN, K, positions, hp, image_of_row=[0] * S, n_mask=n_mask, snapshot_every=every)

        ref, got = serial(), rows()  # warm-up (workspace growth) and the comparison
        same = all(np.array_equal(ref[s][0][:, 0], got[0][:, s]) for s in range(S))
        t_serial, t_rows = [], []
        for _ in range(args.reps):
            for fn, acc in ((serial, t_serial), (rows, t_rows)):
                eng.sync()
                t0 = time.perf_counter()
                fn()
                acc.append(time.perf_counter() - t0)
        rec = dict(logit_scale=scale, precision=runtime.PRECISION_NAMES[prec], S=S, L=L, K=K, sweeps=args.sweeps, order="shuffle",
                   wall_s_serial=t_serial, wall_s_rows=t_rows, captions_per_s_serial=S / min(t_serial), captions_per_s_rows=S / min(t_rows),
                   speedup_best=min(t_serial) / min(t_rows), rows_faster_in_every_rep=all(r < s for r, s in zip(t_rows, t_serial)),
                   ids_identical=bool(same))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    eng.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
