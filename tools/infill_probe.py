#!/usr/bin/env python3
"""N caption templates with unequal blank counts on ONE image: N one-caption runtime.run_infill calls against one run_infill
call over all of them (rows of czc_generate_rows_from calls, one per token length, a caption with fewer blanks sitting out the
rest of every sweep).  Full-size synthetic towers, K = 200, the precision the runtime picks for the logit scale.

    python tools/infill_probe.py [--N 2 4 8] [--sweeps 10] [--reps 3] [--out profiles/r09_infill_probe.json]

Per N: wall time of both arms, warm (one untimed call of each first), --reps repetitions alternating serial / batched, and
whether the captions of every sweep agree.  Nothing about speed is asserted anywhere; this only records what was measured."""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clip.clip import CLIP  # noqa: E402
from conzic_amd import runtime, synth  # noqa: E402
from conzic_amd.models import SyntheticLM  # noqa: E402
from conzic_amd.text import tokenizers_from_vocab  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, nargs="+", default=[2, 4, 8])
ap.add_argument("--L", type=int, default=10)
ap.add_argument("--K", type=int, default=200)
ap.add_argument("--sweeps", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_infill_probe.json"))
args = ap.parse_args()

from PIL import Image  # noqa: E402

sv = synth.make_vocab()
bcfg, ccfg = synth.bert_base(), synth.clip_b32()
bt, ct = tokenizers_from_vocab(sv)
lm = SyntheticLM(bcfg)
clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, 12), ct)
img = Image.fromarray(synth.make_images_u8(1, ccfg.v_image)[0])
log = logging.getLogger("infill-probe")
regular = [t for t in (sv.bert_tokens[i] for i in np.nonzero(synth.make_token_mask(sv, regular_only=True)[0] > 0)[0])
           if t.isalpha() and len(bt.encode(t)) == 3]
rng = np.random.default_rng(3)
kw = dict(order="sequential", max_iters=args.sweeps, top_k=args.K, temperature=0.1, alpha=0.02, beta=2.0)
out = []
for N in args.N:
    caps = []
    for n in range(N):   # L one-piece words each, 1 + n % L of them blank: one token length, unequal blank counts
        words = [regular[int(i)] for i in rng.integers(0, len(regular), args.L)]
        for p in rng.choice(args.L, 1 + n % args.L, replace=False):
            words[int(p)] = "_"
        caps.append(" ".join(words))

    def serial():
        return [runtime.run_infill([c], ["img"], lm, clip, bt, img, synth.make_token_mask(sv), "Image of a", log, verbose=False, **kw)[0]
                for c in caps]

    def batched():
        return runtime.run_infill(caps, ["img"], lm, clip, bt, img, synth.make_token_mask(sv), "Image of a", log, verbose=False, **kw)

    ref, got = serial(), batched()   # warm-up (workspace growth) and the comparison
    same = all(r[0] == g[0] for r, g in zip(ref, got))
    t_serial, t_batched = [], []
    eng = runtime.get_engine(lm, clip, bt)
    for _ in range(args.reps):
        for fn, acc in ((serial, t_serial), (batched, t_batched)):
            eng.sync()
            t0 = time.perf_counter()
            fn()
            acc.append(time.perf_counter() - t0)
    rec = dict(precision=runtime.PRECISION_NAMES[eng.precision], N=N, L=args.L, K=args.K, sweeps=args.sweeps,
               blanks=[c.split().count("_") for c in caps], wall_s_serial=t_serial, wall_s_batched=t_batched,
               ratio_of_medians=float(np.median(t_serial) / np.median(t_batched)), captions_identical=bool(same))
    print(json.dumps(rec), flush=True)
    out.append(rec)
runtime.evict()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
