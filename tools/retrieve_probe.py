#!/usr/bin/env python3
"""Index search against the HBM streaming rate, and against the vendor library forming the whole score matrix.

    python tools/retrieve_probe.py [--N 65536 1048576] [--Q 1 8 32] [--k 5] [--reps 20] [--out profiles/r10_retrieve_probe.json]

D = 512 (the tiny synthetic towers with proj = 512: the search only reads clip_proj of the engine).  Per (N, Q), after three
warm-up calls of each arm, --reps timed calls per arm, the arms alternated:

  search  czc_index_search with the queries already on the device: query normalisation, the scan fused with the top-k, the
          merge and the one read of the results;
  vendor  for comparison only: torch.topk(q @ X.T, k) in fp32 through the vendor GEMM on pre-normalised rows resident on the
          same device, which forms the [Q, N] score matrix.

Both are host-clock times of a call that ends in a device synchronise (the search's own read; torch.cuda.synchronize).  Reported
per arm: median and (max - min) / median; for the search the index bytes it streams per second, N * D * 4 / median (once per
tile of 32 queries), next to the 6.3 TB/s the device's streaming kernels reach; the ratio vendor / search; and, as the check that
both arms answer the same question, the share of the vendor arm's top-k ids the search returned (random rows are near-ties in
fp32, so a few swaps at the k-th place are expected).  Needs a GPU: there is no fallback."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conzic_amd import harness, native, synth  # noqa: E402

STREAM_TBPS = 6.3

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, nargs="+", default=[65536, 1048576])
ap.add_argument("--Q", type=int, nargs="+", default=[1, 8, 32])
ap.add_argument("--k", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--groups", type=int, default=0, help='engine option "index_groups" (0: chosen by the launcher)')
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_retrieve_probe.json"))
args = ap.parse_args()

import torch  # noqa: E402
if not torch.cuda.is_available():
    raise SystemExit("retrieve_probe needs a GPU")
torch.backends.cuda.matmul.allow_tf32 = False
D = 512
sv = harness.cached_vocab(True)
su = harness.build_synthetic(True, native.PREC_SPLIT, clip_cfg=dataclasses.replace(synth.clip_tiny(len(sv.clip_vocab)), proj=D))
eng = su.engine
eng.set_option("index_groups", args.groups)


def stats(ts):
    ts = np.asarray(ts)
    return float(np.median(ts)), float((ts.max() - ts.min()) / np.median(ts))


out = []
for N in args.N:
    gen = torch.Generator(device="cuda").manual_seed(N)
    X = torch.randn(N, D, device="cuda", generator=gen, dtype=torch.float32)
    eng.index_set(X)
    Xn = X / X.norm(dim=1, keepdim=True)
    del X
    for Q in args.Q:
        q = torch.randn(Q, D, device="cuda", generator=gen, dtype=torch.float32)
        qn = q / q.norm(dim=1, keepdim=True)

        def search():
            t0 = time.perf_counter()
            r = eng.index_search(q, args.k)
            return time.perf_counter() - t0, r

        def vendor():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = torch.topk(qn @ Xn.T, args.k)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, r

        for _ in range(3):
            search(), vendor()
        ts, tv = [], []
        for _ in range(args.reps):
            ts.append(search()[0])
            tv.append(vendor()[0])
        (_, (ids, cos)), (_, ref) = search(), vendor()
        ref_ids = ref.indices.cpu().numpy()
        same = float(np.mean([len(set(ids[i]) & set(ref_ids[i])) / args.k for i in range(Q)]))
        worst = float(np.abs(cos - ref.values.cpu().numpy()).max())
        ms, ss = stats(ts)
        mv, sv_ = stats(tv)
        rec = dict(N=N, D=D, Q=Q, k=args.k, reps=args.reps, index_groups=args.groups, search_ms=ms * 1e3, search_spread=ss,
                   vendor_ms=mv * 1e3, vendor_spread=sv_, index_tb_per_s=N * D * 4 / ms / 1e12, streaming_tb_per_s=STREAM_TBPS,
                   share_of_streaming=N * D * 4 / ms / 1e12 / STREAM_TBPS, vendor_over_search=mv / ms,
                   ids_shared_with_vendor=same, worst_cos_diff_vs_vendor_fp32=worst)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    del Xn
    eng.index_clear()
    torch.cuda.empty_cache()
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
