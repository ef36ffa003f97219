#!/usr/bin/env python3
"""Throughput benchmark of the polishing engine (contract: see the task prompt / DESIGN.md §5).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One *step* = one full `generate_caption` pass over one batch of synthetic images on every rank:
BASELINE.json configs[2] -- 256 random-pixel 224x224 images per GPU, sequential order, L=10,
K=200, I=10 sweeps, alpha=0.02, beta=2.0, tau=0.1, prompt "Image of a" -- including the CLIP
vision encode of the batch (once per image).  value = captions/s of the whole job
(N * 256 * K / max-over-ranks time).  Weak scaling: per-GPU work is fixed; `--total-images N` fixes the TOTAL instead
(strong scaling: BASELINE configs[3] 2048 / configs[4] 512 images split over the ranks by `dist.shard_range`).

A plain run sets up, warms up, times `--steps` steps of the bf16 engine on HF-init weights (logit scale 14.3, the engine
north_star names; no HIP events in the timed region), writes the last timed step's outputs with `--dump-outputs`, and prints
the line: `value`, `ms_per_step`.  `--full` adds everything else, as separate passes after the timed region unless noted:
`roofline` (HIP events around the roofline family inside the timed region, which `value` then includes), the per-class
breakdown and the single-stream pass, the batch-invariance check, `captions_crc32`, a second leg with the SAME steps and
warm-up -- `scale100_mode.value` (= `value_scale100`) = the engine `runtime.choose_precision` selects for the published
checkpoints (logit scale 100: screen-then-refine) --, `box_calibration` and the CPU baseline.  The `--no-*` switches turn
single parts of `--full` off.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0  # dense bf16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: all files together


def f_step(K, T, Tc):
    """Algorithmic FLOPs of one image-position-step as the reference executes it."""
    return K * (Tc * 75.87e6 + 0.52e6) + T * 218.5e6


def caption_flops(L, K, I, P=3):
    T = L + P + 2
    tot = 0.0
    for it in range(I):
        for j in range(L):
            Tc = (P + 2 + j + 1) if it == 0 else T  # first sweep: unfilled [MASK]s are dropped
            tot += f_step(K, T, Tc)
    return tot + 8.7e9


def metric_name(L, K, order, gamma=None, samples=1):
    """BASELINE.json's metric, spelled with the shape this line was actually measured on (the default is its own
    "captions/sec (L=10, K=200, seq order)"; --config 3 is L=15, K=512, shuffle order, 3 samples)."""
    o = {"sequential": "seq", "shuffle": "shuffle"}.get(order, order)
    extra = ("" if gamma is None else f", sentiment gamma={gamma:g}") + ("" if samples <= 1 else f", samples_num={samples}")
    return f"captions/sec (L={L}, K={K}, {o} order{extra})"


def per_caption(total, images, samples=1):
    """A per-step total (FLOPs, ...) of one rank divided by the captions that step produced: images x samples_num."""
    return total / (images * max(1, samples))


def dump_outputs(out_dir, embeds, ids, cos, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: what a caller of the timed path received in the last timed step, one .npy per array --
    image_embeds [B, proj] fp32 (encode_images), ids [samples, snapshots, B, T] as float64 (exact for int32 token ids) and
    cos [samples, snapshots, B] fp32 (generate, one call per sample), image_index [n] float64 = the images written.  All
    images while the files fit in `limit` bytes, else a fixed seeded sample of them (same images on every run)."""
    embeds = np.asarray(embeds, np.float32)
    ids, cos = np.asarray(ids, np.float64), np.asarray(cos, np.float32)
    B = embeds.shape[0]
    per_image = (embeds[0].nbytes + ids[:, :, 0].nbytes + cos[:, :, 0].nbytes + 8)
    n = min(B, max(1, (limit - 4096) // per_image))  # 4 KiB: the .npy headers
    keep = np.arange(B) if n == B else np.sort(np.random.default_rng(0).choice(B, size=n, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    arrays = dict(image_embeds=embeds[keep], ids=ids[:, :, keep], cos=cos[:, :, keep], image_index=keep.astype(np.float64))
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(arr))
    return sum(arr.nbytes for arr in arrays.values())


def physical_cores():
    """Physical cores of this host (distinct (package, core) pairs of /proc/cpuinfo), or None."""
    try:
        seen, pkg = set(), 0
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("physical id"):
                pkg = int(ln.split(":")[1])
            elif ln.startswith("core id"):
                seen.add((pkg, int(ln.split(":")[1])))
        return len(seen) or None
    except OSError:
        return None


CPU_BASELINE_THREADS = 16


def box_calibration():
    """How fast THIS box is, with nothing of this repo in it: a dense bf16 torch.matmul (hipBLASLt) of 8192^3, TFLOP/s.  The boxes of
    the pool differ by several per cent on identical code (clocks under load, host); lines from different boxes compare through it."""
    import torch
    try:
        a = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
        b = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
        for _ in range(3):
            a @ b
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            a @ b
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20
        return dict(what="torch.matmul bf16 8192 x 8192 x 8192 (vendor library), mean of 20 after 3", ms=round(ms, 4),
                    tflops=round(2.0 * 8192 ** 3 / (ms * 1e-3) / 1e12, 1))
    except Exception as exc:  # the measurement is a courtesy figure, never a reason to lose the line
        return dict(what="torch.matmul bf16 8192^3", error=str(exc)[:200])


def cpu_baseline(L, K, I=10, threads=None):
    """The oracle (CPU restatement of the reference, oracle/) timed on this host: B=1, config-1 shape, ONE FULL caption
    (image encode + I sweeps x L position-steps, nothing extrapolated).  Thread count: fixed at
    min(CPU_BASELINE_THREADS, physical cores) -- plain torch at B = 1 shapes (3000 x 512 GEMMs) peaks there on the GPU boxes'
    hosts (rounds 1-4 swept 8..256 threads on them: 16 was fastest every time, 0.40 s per full-length position-step; 128
    threads 1.7 s, all 256 threads 64 s) and a fixed count takes the sweep's noise out of the figure; --cpu-threads overrides."""
    import torch
    from conzic_amd import synth
    from oracle import models as M, step as S, text as T
    sv = synth.make_vocab()
    bcfg, ccfg = synth.bert_base(), synth.clip_b32()
    o = S.Oracle(M.to_torch(synth.make_bert_weights(bcfg, 11)), bcfg, M.to_torch(synth.make_clip_weights(ccfg, 12)),
                 ccfg, sv.bert_tokens, T.ClipBpe(sv.clip_vocab, sv.clip_merges))
    mask = torch.from_numpy(synth.make_token_mask(sv, regular_only=True))
    pix = synth.pixels_from_u8(synth.make_images_u8(1))
    ncpu, phys = os.cpu_count() or 8, physical_cores()
    from conzic_amd.dist import local_world_size
    threads = int(threads) if threads else max(1, min(CPU_BASELINE_THREADS, (phys or ncpu) // local_world_size()))
    torch.set_num_threads(threads)
    with torch.no_grad():
        # warm the thread pool and the allocator on one full-length step (untimed)
        regular = np.nonzero(mask[0].numpy() > 0)[0]
        probe = torch.tensor(o.init_text("Image of a", L, 1))
        probe[:, 4:4 + L] = torch.from_numpy(np.random.default_rng(0).choice(regular, size=(1, L)))
        emb0 = o.image_embeds(pix)
        probe[:, 4 + L // 2] = o.mask_id
        S.polish_step(o, probe, emb0, mask, 4 + L // 2, K, 0.1, 0.02, 2.0)
        t_start = time.time()
        emb = o.image_embeds(pix)
        t_img = time.time() - t_start
        inp = torch.tensor(o.init_text("Image of a", L, 1))
        ts = []
        for sw in range(I):
            t0 = time.time()
            for ii in range(L):
                o.update_token_mask(mask, L, ii)
                inp[:, 4 + ii] = o.mask_id
                S.polish_step(o, inp, emb, mask, 4 + ii, K, 0.1, 0.02, 2.0)
            ts.append(time.time() - t0)
        t_caption = time.time() - t_start
    return dict(value=1.0 / t_caption, unit="captions/s", cores=threads, kind="port",
                host=dict(logical_cpus=ncpu, physical_cores=phys),
                sample=f"oracle (plain torch fp32) B=1 L={L} K={K} I={I} on {threads} threads of this host ({phys} physical cores, "
                       f"{ncpu} logical): ONE FULL caption timed end to end = {t_caption:.1f}s (image encode {t_img:.2f}s, sweeps "
                       + ", ".join(f"{t:.2f}" for t in ts) + " s); nothing extrapolated")


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N ranks of this same command (rank r <-> GPU r, RCCL over
    xGMI, rendezvous on 127.0.0.1), relay rank 0's JSON line, fail if any rank fails.  Never falls back to fewer GPUs."""
    import socket
    import subprocess
    import torch
    have = torch.cuda.device_count()
    share = os.environ.get("CZC_SHARE_GPU") == "1"
    if have < n and not share:
        print(f"bench.py: --gpus {n} needs {n} visible GPUs, found {have} (no silent fallback to fewer GPUs; "
              f"--share-gpu exists for single-device tests of the N-rank path only)", file=sys.stderr, flush=True)
        return 2
    if have < 1:
        print("bench.py: no GPU visible (the engine has no CPU fallback)", file=sys.stderr, flush=True)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        if share and have < n:
            env["CZC_DIST_BACKEND"] = "gloo"
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rcs = [p.wait() for p in procs]
    bad = [(r, c) for r, c in enumerate(rcs) if c != 0]
    if bad:
        print(f"bench.py: ranks failed (rank, exit code): {bad}", file=sys.stderr, flush=True)
        return 1
    return 0


# BASELINE.json configs[1..4] as flag presets (explicit flags still win): what the driver's SCALE runs would launch
CONFIG_PRESETS = {
    1: dict(images=1),                                                              # configs[1]: single image, L=10 K=200 sequential
    2: dict(images=256),                                                            # configs[2]: 256 images on one GPU (the default)
    3: dict(total_images=2048, order="shuffle", L=15, topk=512, samples=3),         # configs[3]: 2048 images over the ranks, 3 samples
    4: dict(total_images=512, gamma=5.0, L=12, topk=200),                           # configs[4]: controllable run, 512 images
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=None, choices=sorted(CONFIG_PRESETS),
                    help="BASELINE.json configs[N] as a preset of the flags below (explicit flags override it): "
                         "1 single image; 2 256 images (default); 3 --total-images 2048 --order shuffle --len 15 --topk 512 --samples 3; "
                         "4 --total-images 512 --gamma 5 --len 12")
    ap.add_argument("--samples", type=int, default=1,
                    help="samples_num (demo.py:83, run.py:180): polish every image this many times per step; the images are "
                         "encoded ONCE per step and the embeddings re-used (north_star's cached image encode); in shuffle order "
                         "every sample draws its own order from the one random.Random(42) stream, as the reference's loop does")
    ap.add_argument("--control", default="table", choices=["table", "exact", "both"],
                    help="with --gamma: where the control scores come from -- `table` a synthetic per-token sentiment table inside "
                         "the bridge kernel (the approximate throughput mode), `exact` the product's HostScorer (the reference's "
                         "sentence scorer, called back per step under the CLIP tower) over tests/nltk_standin.py installed as nltk "
                         "with CZC_STANDIN_COST_US of busy CPU per 12-word sentence (default 300: roughly nltk's perceptron "
                         "tagger), `both` = table as the headline leg and exact as a second leg")
    ap.add_argument("--cpu-threads", type=int, default=None, help="threads of the CPU baseline (default min(16, physical cores))")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images", type=int, default=256, help="images per GPU per step (configs[2]: 256)")
    ap.add_argument("--len", type=int, default=10, dest="L")
    ap.add_argument("--topk", type=int, default=200)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--order", default="sequential", choices=["sequential", "shuffle"])
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f32", "split", "fp16", "refine"])
    ap.add_argument("--logit-scale", type=float, default=2.6592, help="CLIP logit_scale (HF init 2.6592; published checkpoint ln 100 = 4.6052)")
    ap.add_argument("--gamma", type=float, default=None, help="sentiment control weight (BASELINE configs[4]: 5.0)")
    ap.add_argument("--sentiment", default="positive", choices=["positive", "negative"])
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline figure: roofline and per-kernel figures, batch "
                         "invariance, captions_crc32, the scale-100 leg, box_calibration, the CPU baseline (the --no-* switches "
                         "below turn single parts off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (image_embeds, ids, cos of every image; "
                         "rank 0 gathers the ranks' images) as DIR/<name>.npy, float32 / float64, 64 MB at most")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-profile", action="store_true", help="with --full: skip the HIP-event kernel timing (roofline)")
    ap.add_argument("--no-alt", action="store_true", help="with --full: skip the second leg (the engine the product path selects at the published logit scale)")
    ap.add_argument("--alt-steps", type=int, default=None,
                    help="timed steps of the scale-100 leg (default: --steps, with --warmup warm-up steps: both legs on equal footing)")
    ap.add_argument("--total-images", type=int, default=None,
                    help="strong scaling: polish this many images in total, split over the ranks by dist.shard_range "
                         "(BASELINE configs[3]: 2048, configs[4]: 512); default: --images per GPU (weak scaling)")
    ap.add_argument("--alt-split", action="store_true", help="also time the all-split-fp16 engine at the published logit scale (the round-2 product mode)")
    ap.add_argument("--no-invariance", action="store_true", help="with --full: skip the batch-invariance check after the timed loop")
    ap.add_argument("--streams", type=int, default=2,
                    help="concurrent image sub-batches per GPU, each on its own HIP stream over the same weights "
                         "(czc_replicate); 1 = one engine, one stream")
    ap.add_argument("--min-images", type=int, default=32, help="images per stream below which a batch is not split")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=INT", help="engine option (czc_set_option), A/B runs")
    ap.add_argument("--share-gpu", action="store_true",
                    help="TEST ONLY: allow --gpus N ranks on fewer than N devices (rank r -> device r %% count, gloo rendezvous: "
                         "RCCL cannot put two ranks on one device).  Such a line says so in config.parallelism")
    pre, _ = ap.parse_known_args()
    if pre.config is not None:
        ap.set_defaults(**CONFIG_PRESETS[pre.config])
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if not a.full:  # a plain run: the timed steps of the headline leg and nothing else
        a.no_cpu_baseline = a.no_profile = a.no_alt = a.no_invariance = True
    if a.share_gpu:
        os.environ["CZC_SHARE_GPU"] = "1"
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(a.gpus))  # plain `python bench.py --gpus N`: this process becomes the launcher of N ranks

    import torch
    from conzic_amd import dist as czd
    from conzic_amd import harness, native, synth
    from conzic_amd.engine import Engine, EngineGroup

    rank, world, local = czd.env_rank_world()
    if world != a.gpus:
        sys.exit(f"bench.py: WORLD_SIZE={world} but --gpus {a.gpus}: the launcher's rank count and --gpus must agree")
    assert torch.cuda.is_available(), "bench.py needs a GPU (the engine has no CPU fallback)"
    shared_gpu = torch.cuda.device_count() < world
    if shared_gpu and os.environ.get("CZC_SHARE_GPU") != "1":
        sys.exit(f"bench.py: {world} ranks but {torch.cuda.device_count()} visible GPUs (one rank per GPU; --share-gpu is for tests)")
    local = local % torch.cuda.device_count()
    # host resources per rank: CPU affinity = this rank's slice of its GPU's NUMA node, torch threads to match (no-op at one rank)
    host_info = czd.pin_rank(int(os.environ.get("LOCAL_RANK", 0)), device_index=local)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    backend = os.environ.get("CZC_DIST_BACKEND", "nccl")  # "nccl" == RCCL on ROCm
    dist_world = None
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        dist_world = dist.get_world_size()  # what the collective backend itself counts
        assert dist_world == a.gpus, (dist_world, a.gpus)

    prec = {"bf16": native.PREC_BF16, "f32": native.PREC_F32, "split": native.PREC_SPLIT, "fp16": native.PREC_FP16,
            "refine": native.PREC_REFINE}[a.precision]
    DT = {native.PREC_BF16: "bf16", native.PREC_F32: "f32", native.PREC_FP16: "fp16",
          native.PREC_SPLIT: "split-fp16 (fp16 hi+lo planes, 3 MFMA passes, fp32 accumulate)",
          native.PREC_REFINE: "fp16 screening pass + split-fp16 refine pass (fp32 accumulate)"}
    if a.alt_steps is None:
        a.alt_steps = a.steps  # both legs: the same steps and warm-up
    a.alt_warmup = a.warmup
    B, L, K, I = a.images, a.L, a.topk, a.iters
    if a.total_images is not None:
        lo, hi = czd.shard_range(a.total_images, rank, world)  # strong scaling: the total is fixed, ranks own contiguous shards
        B = hi - lo
        if B < 1:
            sys.exit(f"bench.py: --total-images {a.total_images} leaves rank {rank} of {world} without an image")
    else:
        lo = rank * B  # weak scaling: rank r polishes images [r*B, (r+1)*B)
    n_total = a.total_images if a.total_images is not None else world * B
    u8 = synth.make_images_u8(B, first=lo)
    pixels = torch.from_numpy(synth.pixels_from_u8(u8)).to(dev)  # resident in HBM before the clock starts
    seed_len = 4
    # one visiting order per sample (gen_utils.py:110-111: one random.shuffle per call from the process-global stream,
    # seeded once -- demo.py:107 -- and NOT reseeded between samples, demo.py:83)
    sample_plans = []
    import random
    order_rng = random.Random(42)
    for _ in range(max(1, a.samples)):
        order_list = None
        if a.order == "shuffle":
            order_list = list(range(L))
            order_rng.shuffle(order_list)
        sample_plans.append(harness.order_positions(a.order, L, I, order_list=order_list))
    pos, nm, every = sample_plans[0]
    hp = Engine.hyper(0.02, 2.0, 0.1, a.gamma, a.sentiment == "negative")

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    def run_mode(prec_, logit_scale, steps, warmup, profile, opts=(), invariance=False, control="table", dump_dir=None):
        """Engine in one precision at one logit scale: warm up, time `steps` passes, return the measurements (with
        `dump_dir`: write the last timed pass's outputs there first)."""
        exact = a.gamma is not None and control == "exact"
        bcfg, ccfg = synth.bert_base(), synth.clip_b32()
        ccfg.logit_scale = logit_scale  # make_clip_weights writes it into the "logit_scale" tensor
        # frozen weights: generated on rank 0, broadcast once over RCCL (xGMI), consumed in place
        t0 = time.time()
        broadcast_s = None
        if world > 1:
            bw_src = synth.make_bert_weights(bcfg, 11) if rank == 0 else None
            cw_src = synth.make_clip_weights(ccfg, 12) if rank == 0 else None
            barrier()
            tb = time.perf_counter()
            bw = czd.broadcast_state(bw_src, dev)
            cw = czd.broadcast_state(cw_src, dev)
            barrier()
            broadcast_s = round(time.perf_counter() - tb, 4)   # both towers' buckets, rank 0's host arrays -> every GPU
            del bw_src, cw_src
        else:
            bw, cw = synth.make_bert_weights(bcfg, 11), synth.make_clip_weights(ccfg, 12)
        su = harness.build_synthetic(False, prec_, logit_scale=logit_scale, regular_only=True, device=local, bert_w=bw,
                                     clip_w=cw, bert_cfg=bcfg, clip_cfg=ccfg, lexicon=a.gamma is not None and not exact)
        del bw, cw
        eng = su.engine
        scorer = None
        if exact:
            # the product's exact control mode: conzic_amd.control.HostScorer (the reference's sentence scorer,
            # sentiments_classifer.py:9-33) called back by the engine once per step WHILE the step's CLIP tower runs; nltk
            # itself exists on neither box, so the tagger is tests/nltk_standin.py with a calibrated busy-CPU cost
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import nltk_standin
            from conzic_amd import control as czcontrol
            os.environ.setdefault("CZC_STANDIN_COST_US", "300")
            nl = nltk_standin.install()
            env_w = os.environ.get("CZC_CONTROL_WORKERS", "").strip()
            scorer = czcontrol.HostScorer(su.bert_tok, "sentiment", a.sentiment, nl, workers=int(env_w) if env_w else None,
                                          worker_hook=nl.__worker_hook__)
            eng.set_control_callback(scorer)
        for kv in opts:
            k, v = kv.split("=")
            if k.startswith("test:"):  # kernel-level A/B switches (czc_test_set_option)
                assert native.load_test().czc_test_set_option(k[5:].encode(), int(v)) == 0, k
            else:
                eng.set_option(k, int(v))
        # the images are polished as `streams` contiguous sub-batches, each by its own engine replica (same weights, own
        # stream) driven from its own host thread: same captions image for image (tests/test_streams_gpu.py), and one
        # sub-batch's small launches and GEMM tail rounds overlap the other's big launches
        grp = EngineGroup(eng, streams=a.streams, min_images=a.min_images)
        n_streams = len(grp.parts(B))
        t_setup = time.time() - t0
        init = su.bert_tok.encode("Image of a" + su.bert_tok.mask_token * L)

        last = {}

        per_step_scoring = []

        def step():
            if scorer is not None:
                # every step polishes the SAME resident images: a memo kept across steps would hand the timed steps the
                # strings the warm-up (or the previous step) already scored.  A real run sees new images per batch, so each
                # step starts cold; what remains is the reuse INSIDE one generate call (same candidates at a position whose
                # context did not change between sweeps)
                with scorer._lock:
                    scorer.sent_memo.clear()
                a0, s0 = scorer.asked, scorer.scored
            last["embeds"] = grp.encode_images(pixels)  # once per image and step; every sample re-uses the resident embeddings
            last["gen"] = [grp.generate(B, init, L, seed_len, K, sp, hp, n_mask=sn, snapshot_every=se) for sp, sn, se in sample_plans]
            out_ = last["gen"][-1]
            if scorer is not None:
                per_step_scoring.append((scorer.asked - a0, scorer.scored - s0))
            return out_

        for _ in range(warmup):
            step()
        grp.profile_reset()
        # timed region: HIP events only around the roofline kernel family (an event pair around EVERY kernel costs 3 %
        # at B = 256 and 37 % at B = 1); the per-class breakdown comes from one extra, untimed, fully profiled step
        # the event pairs around the CLIP-text tower's launches cost 0-1 % of a step at 256 images but 4.5 % at 64, 7.5 % at 32,
        # 18 % at 8 and 30-45 % at one image (a chain of ~200 launches of 5-15 us): below 128 images per GPU the timed region
        # runs WITHOUT events and the tower's figures come from ONE extra pass of the same step
        events_in_region = profile and B >= 128
        grp.profile(2 if events_in_region else 0)
        barrier()
        del per_step_scoring[:]
        host_s0 = scorer.host_seconds if scorer is not None else 0.0
        t0 = time.perf_counter()
        for _ in range(steps):
            ids, cos = step()
        barrier()
        dt = time.perf_counter() - t0
        timed_scoring = list(per_step_scoring)
        if dump_dir is not None:
            embeds_ = last["embeds"]
            ids_ = np.stack([g_[0] for g_ in last["gen"]])
            cos_ = np.stack([g_[1] for g_ in last["gen"]])
            if world > 1:  # every rank's images, in image order (shard order = rank order)
                embeds_ = czd.gather_along(embeds_, world, axis=0)
                ids_ = czd.gather_along(ids_, world, axis=2)
                cos_ = czd.gather_along(cos_, world, axis=2)
            if rank == 0:
                nbytes = dump_outputs(dump_dir, embeds_, ids_, cos_)
                print(f"bench.py: wrote {nbytes / 2 ** 20:.1f} MB of outputs of the last timed step to {dump_dir}",
                      file=sys.stderr, flush=True)
        host_s_timed = (scorer.host_seconds - host_s0) if scorer is not None else 0.0
        grp.profile(False)
        stats = grp.stats()
        prof_steps = steps
        if profile and not events_in_region:
            grp.profile_reset()
            grp.profile(2)
            step()
            grp.profile(False)
            prof_steps = 1
        per_rank = [(B, dt)]
        if world > 1:
            import torch.distributed as dist
            t = torch.tensor([float(B), dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            allt = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(allt, t)  # every rank's own image count and wall time: a straggler shows up per rank
            per_rank = [(int(x[0].item()), float(x[1].item())) for x in allt]
            dt = max(d for _, d in per_rank)
        kinds = ["gemm_clip_text", "gemm_clip_refine", "attention_clip_text", "rowops_clip_text", "gemm_bert", "gemm_vision",
                 "attention", "rowops", "topk", "bridge", "combine"]
        fam = ("gemm_clip_text", "gemm_clip_refine")  # the roofline family (the second only exists in the refine engine)
        tower = fam + ("attention_clip_text", "rowops_clip_text")  # everything the CLIP-text K-candidate batch runs
        prof_timed = {k: grp.profile_get(k) for k in tower} if profile else {}
        if profile:  # time the GPU spent in ANY kernel of the text tower (union over classes and streams)
            from conzic_amd.engine import union_ms
            prof_timed["_tower_busy_ms"] = union_ms([e_.profile_intervals(k, grp.engines[0]) for e_ in grp.engines for k in tower])
        prof, breakdown, single_ms = prof_timed, {}, None

        def single_step():  # the same step on ONE engine and ONE stream (all B images in every launch)
            eng.encode_images(pixels)
            for sp, sn, se in sample_plans:
                out_ = eng.generate(B, init, L, seed_len, K, sp, hp, n_mask=sn, snapshot_every=se)
            return out_

        if profile:
            if n_streams > 1:
                # roofline pass: with concurrent sub-batches a launch's duration includes the time its kernel shared the
                # chip with the other stream's kernels (of every class), so it no longer says how good the kernel is;
                # the kernel-quality figure comes from one extra pass of the same step on one stream, the contended
                # figures of the timed region are reported beside it
                eng.profile_reset()
                eng.profile(2)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                single_step()
                eng.sync()
                single_ms = (time.perf_counter() - t1) * 1e3
                eng.profile(False)
                prof = {k: eng.profile_get(k) for k in tower}
            eng.profile_reset()
            eng.profile(1)
            single_step()
            eng.profile(False)
            breakdown = {k: eng.profile_get(k) for k in kinds}
        # the captions of the last timed step over ALL ranks (image order = rank order = shard order), as a checksum: an N-rank
        # strong-scaling run must reproduce the 1-rank run's ids exactly (tests/test_dist_gpu.py)
        ids_crc = gather_s = None
        if a.full:
            import zlib
            tg = time.perf_counter()
            all_ids = czd.gather_along(ids, world, axis=1) if world > 1 else ids
            gather_s = round(time.perf_counter() - tg, 4) if world > 1 else None
            ids_crc = zlib.crc32(np.ascontiguousarray(all_ids, dtype=np.int32).tobytes()) & 0xFFFFFFFF
        ctl = None
        if scorer is not None:
            ctl = dict(scorer="conzic_amd.control.HostScorer over tests/nltk_standin.py installed as nltk (a stand-in: nltk and its "
                              "corpora exist on neither box); context-dependent tagger, the reference's arithmetic",
                       cost_us_per_12_word_sentence=float(os.environ.get("CZC_STANDIN_COST_US", "0")),
                       workers=scorer.workers, host_cpus=os.cpu_count(), callbacks=scorer.calls,
                       timed_steps=[dict(sentences_asked=a_, sentences_scored=s_) for a_, s_ in timed_scoring],
                       sentences_asked=sum(a_ for a_, _ in timed_scoring), sentences_scored=sum(s_ for _, s_ in timed_scoring),
                       memo_hit_frac=round(1.0 - sum(s_ for _, s_ in timed_scoring) / max(sum(a_ for a_, _ in timed_scoring), 1), 4),
                       memo="sentence memo EMPTIED at the start of every step (warm-up and timed): the hit fraction is reuse inside one "
                            "generate call only, what a run over new images per batch sees",
                       host_seconds_in_scorer=round(host_s_timed, 2),
                       note="the callback runs on the host while the same step's CLIP tower runs on the GPU (csrc/engine.hip "
                            "control_score); counts and host_seconds_in_scorer cover the TIMED steps only (summed over the streams' threads)")
            scorer.close()
        res = dict(host=host_info, broadcast_s=broadcast_s, gather_s=gather_s, dt=dt, prof=prof, prof_timed=prof_timed, breakdown=breakdown, stats=stats, setup_s=t_setup, invariance=None, control=ctl,
                   streams=n_streams, single_ms=single_ms, per_rank=per_rank, steps=prof_steps, events_in_region=events_in_region, ids_crc=ids_crc,
                   n_ids=n_total)
        if invariance and rank == 0 and B > 2:
            # batch invariance: images 0-1 encoded and polished ALONE (B = 2) by the same engine must come out as they did
            # inside the batch of B (per-image work is independent: gen_utils.py:65-81 has no cross-image term), with no
            # kernel switches: the pair takes the tiled GEMMs, the LayerNorm kernel and the per-group attention kernel where
            # the batch took the ring / full-row GEMMs and the per-image attention kernel, and every kernel that can serve
            # a layer produces the same bits (tests/test_kernels_gpu.py, test_step_gpu.py::test_caption_does_not_depend_on_the_batch)
            emb2 = eng.encode_images(pixels[:2])
            sp, sn, se = sample_plans[-1]  # `ids` are the last sample's
            ids2, cos2 = eng.generate(2, init, L, seed_len, K, sp, hp, n_mask=sn, snapshot_every=se)
            same = (ids2 == ids[:, :2]).mean(axis=(0, 2))
            res["invariance"] = dict(images=2, batch=B, kernel_switches="none", identical_token_frac=[round(float(x), 4) for x in same],
                                     final_ids_identical=[bool((ids2[-1, j] == ids[-1, j]).all()) for j in range(2)],
                                     max_abs_cos_diff=round(float(np.abs(cos2 - cos[:, :2]).max()), 6),
                                     image_embeds_identical=bool((emb2 == last["embeds"][:2]).all()))
        grp.close()
        return res

    main_res = run_mode(prec, a.logit_scale, a.steps, a.warmup, not a.no_profile, opts=a.opt,
                        invariance=not a.no_invariance, control="exact" if a.control == "exact" else "table",
                        dump_dir=a.dump_outputs)
    exact_res = None
    if a.gamma is not None and a.control == "both":
        exact_res = run_mode(prec, a.logit_scale, a.steps, a.warmup, False, opts=a.opt, control="exact")
    alt_res = split_res = None
    if not a.no_alt and prec == native.PREC_BF16 and a.logit_scale < 4.0:
        # the engine the product path selects for the published checkpoints (logit_scale = ln 100): screen-then-refine,
        # same steps and warm-up as the headline leg at the defaults (bounded when the caller asks for many steps)
        alt_res = run_mode(native.PREC_REFINE, 4.6052, a.alt_steps, a.alt_warmup, not a.no_profile)
        if a.alt_split:
            split_res = run_mode(native.PREC_SPLIT, 4.6052, a.alt_steps, a.alt_warmup, not a.no_profile)

    def refine_block(st_):
        return dict(candidate_seqs=st_["clip_seqs"], re_encoded=st_["refine_seqs"],
                    re_encoded_frac=round(st_["refine_seqs"] / max(st_["clip_seqs"], 1), 4),
                    rows=st_["clip_rows"], re_encoded_rows=st_["refine_rows"],
                    image_steps=st_["gate_image_steps"], gated_image_steps=st_["gated_image_steps"],
                    gated_frac=round(st_["gated_image_steps"] / max(st_["gate_image_steps"], 1), 4),
                    gate="czc_generate margin gate (include/conzic_hip.h czc_refine_gate_stats): image-steps whose screening winner "
                         "survives every cosine-error assignment within delta skip the second pass (delta = 4e-4 x 1.75: the screening pass of czc_generate runs on fp16 rows, option refine_rows16) (winner re-encoded at "
                         "snapshot steps only, for the returned cosine); the others take the full selection")

    def family_of(prof, passes):
        """Executed MFMA work and event time of the CLIP-text linear layers (screening GEMMs: `passes` MFMA passes per
        product; the refine pass's split-fp16 GEMMs: three)."""
        g = dict(prof["gemm_clip_text"])
        g["flops"] *= passes
        g.setdefault("busy_ms", g["ms"])
        r = prof.get("gemm_clip_refine")
        if r and r["launches"]:
            g = dict(ms=g["ms"] + r["ms"], launches=g["launches"] + r["launches"], flops=g["flops"] + 3 * r["flops"],
                     busy_ms=g["busy_ms"] + r.get("busy_ms", r["ms"]))
        return g, (r if r and r["launches"] else None)

    def tower_util(prof, passes, peak, busy_ms=None):
        """north_star's quantity: MFMA utilisation of the whole CLIP-text K-candidate batch = executed FLOPs of its linear
        layers AND its attention / (time in ALL of its kernels: GEMMs, attention, LayerNorm / embedding / gathers) / peak."""
        g, _ = family_of(prof, passes)
        at, ro = prof.get("attention_clip_text"), prof.get("rowops_clip_text")
        if not at or not at["launches"]:
            return None
        fl = g["flops"] + passes * at["flops"]
        ms = busy_ms if busy_ms else g["ms"] + at["ms"] + ro["ms"]
        return dict(frac=round(fl / (ms * 1e-3) / 1e12 / peak, 4), executed_tflop=round(fl / 1e12, 2), kernel_ms=round(ms, 1),
                    gemm_ms=round(g["ms"], 1), attention_ms=round(at["ms"], 1), rowops_ms=round(ro["ms"], 1),
                    attention_tflop=round(passes * at["flops"] / 1e12, 2))

    def roofline_of(res, prec_):
        pt, ps = res["prof_timed"], res["prof"]
        if not pt or not pt["gemm_clip_text"]["launches"]:
            return None
        passes = 3 if prec_ == native.PREC_SPLIT else 1  # split-fp16: every product is three fp16 MFMA passes
        peak = 157.3 if prec_ == native.PREC_F32 else PEAK_BF16_TFLOPS
        g, r = family_of(pt, passes)
        # the figures below divide out of the SAME execution `value` is timed on: executed FLOPs of the family in the
        # timed region / the time the GPU spent on the family there (union of its launch intervals over the streams)
        ach = g["flops"] / (g["busy_ms"] * 1e-3) / 1e12
        # HBM bytes per launch come from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this same
        # command (not measurable inside the run); only quoted for the workload and precision they were taken on
        traffic, src = None, None
        key = {native.PREC_BF16: "bf16", native.PREC_REFINE: "refine"}.get(prec_)
        for tp in ("r06_bench_gemm_traffic.json", "r05_bench_gemm_traffic.json", "r04_bench_gemm_traffic.json", "r03_bench_gemm_traffic.json"):
            tp = os.path.join(ROOT, "profiles", tp)
            if key and os.path.exists(tp) and (a.images, L, K, I, a.order, a.gamma, a.total_images) == (256, 10, 200, 10, "sequential", None, None):
                tj = json.load(open(tp))
                if key in tj:
                    traffic = tj[key]["hbm_bytes_per_launch"]
                    src = (f"profiles/{os.path.basename(tp)} (tools/probes/pmc_bench_traffic.sh: separate rocprofv3 --pmc FETCH_SIZE / "
                           "WRITE_SIZE passes over one caption batch of this workload, gfx950 FETCH_SIZE x2 correction)")
                    break
        fused = not any(kv.replace(" ", "") == "fuse_ln=0" for kv in a.opt)
        r16 = not any(kv.replace(" ", "") == "resid16=0" for kv in a.opt)  # bf16 engine: fp16 residual stream (engine option resid16)
        half = ("CLIP-text linear layers: czc::gemm_wreg_kernel<%s> (qkv, fc1; weights in registers) + "
                + ("czc::gemm_rowln_kernel<%s> (out-proj on full 512-wide rows; its launches also do the LayerNorm that follows) + "
                   "czc::gemm256x_kernel<%s> (fc2; 256x256 LDS-DMA ring, two wave groups one phase apart)" if fused else
                   "czc::gemm256x_kernel<%s> (out-proj, fc2; 256x256 LDS-DMA ring, two wave groups one phase apart)"))
        half16 = ("CLIP-text linear layers on a 2-byte (fp16) residual stream: czc::gemm_wreg_kernel<bf16> (qkv, fc1; weights in registers) + "
                  "czc::gemm_wreg_resid_kernel<bf16> (out-proj; weights in registers, residual rows through per-wave LDS tiles, x updated "
                  "in place) + czc::gemm256x_kernel<bf16, x16 epilogue> (fc2; 256x256 LDS-DMA ring, two wave groups one phase apart)")
        kern = {native.PREC_BF16: half16 if r16 else half % (("bf16",) * (3 if fused else 2)),
                native.PREC_FP16: half % (("fp16",) * (3 if fused else 2)),
                native.PREC_SPLIT: "CLIP-text linear layers: czc::gemm256sq_kernel (split-fp16 operands, 256x256 LDS-DMA ring, three "
                                   "v_mfma_f32_32x32x16_f16 per product)",
                native.PREC_F32: "CLIP-text linear layers: czc::gemm_kernel<float> (v_mfma_f32_32x32x2_f32)"}
        kern[native.PREC_REFINE] = ("screening pass: " + kern[native.PREC_FP16] + "; refine pass (the candidates that carry the "
                                    "softmax_K mass): " + kern[native.PREC_SPLIT])
        out = dict(bound="mfma", kernel=kern[prec_], achieved=round(ach, 1), peak=peak, unit="TFLOP/s", frac=round(ach / peak, 4),
                   traffic=traffic, traffic_source=src, launches=g["launches"],
                   avg_launch_ms=round(g["ms"] / g["launches"], 4), family_busy_ms_per_step=round(g["busy_ms"] / res["steps"], 1),
                   flops_per_launch=g["flops"] / g["launches"], mfma_passes_per_product=passes,
                   measured_on=(("the timed region" if res.get("events_in_region", True) else
                                 "ONE extra pass of the same step right after the timed region (fewer than 128 images per GPU: the event "
                                 "pairs would cost 4-45 % of the step, so the timed region carries none)")
                                + ": HIP events on each engine's own stream around every launch of the family; "
                                + ("achieved = executed FLOPs / the UNION of the family's launch intervals over the %d streams (the time "
                                   "the GPU spent on the family; a launch's own duration there -- avg_launch_ms, what rocprofv3 --stats of "
                                   "this command reports -- includes the time it shared the chip with the other stream's kernels)"
                                   % res["streams"] if res["streams"] > 1 else "achieved = executed FLOPs / the sum of the launch durations")),
                   refine_pass=None if not r else dict(
                       launches=r["launches"], ms=round(r["ms"], 1), mfma_tflop=round(3 * r["flops"] / 1e12, 2),
                       share_of_family_time=round(r["ms"] / g["ms"], 3)),
                   clip_text_mfma_util=tower_util(pt, passes, peak, pt.get("_tower_busy_ms")))
        if out["clip_text_mfma_util"]:
            out["clip_text_mfma_util"]["note"] = ("executed FLOPs of the CLIP-text linear layers + attention (4 * hidden * causal (query, key) pairs "
                                                   "per layer) / the time the GPU spent in ANY CLIP-text kernel in the timed region (GEMMs, attention, "
                                                   "LayerNorm / embedding / gathers; union over classes and streams) / peak -- north_star's "
                                                   "'MFMA utilisation on the CLIP-text K-candidate batch' (target 0.40)")
        if res["streams"] > 1 and ps is not pt and ps.get("gemm_clip_text", {}).get("launches"):
            g1, _ = family_of(ps, passes)
            a1 = g1["flops"] / (g1["ms"] * 1e-3) / 1e12
            out["single_stream_pass"] = dict(
                achieved=round(a1, 1), frac=round(a1 / peak, 4), avg_launch_ms=round(g1["ms"] / g1["launches"], 4), launches=g1["launches"],
                clip_text_mfma_util=tower_util(ps, passes, peak),
                note="kernel-quality figure: one extra pass of the same step on ONE engine / ONE stream right after the timed region "
                     "(every launch carries all the images and runs alone on the GPU); rocprofv3 --stats of `bench.py --streams 1` agrees with it")
        return out

    if rank == 0:
        captions = n_total * a.steps * max(1, a.samples)
        value = captions / main_res["dt"]
        prof, st = main_res["prof"], main_res["stats"]
        if (L, K, I, a.order, a.gamma) == (10, 200, 10, "sequential", None):
            cfg_name = "BASELINE configs[2]" if B > 1 else "BASELINE configs[1] (single image)"
        elif (L, K, a.order, a.gamma) == (15, 512, "shuffle", None):
            cfg_name = "BASELINE configs[3] shape (per-GPU shard)"
        elif a.gamma is not None and L == 12 and K == 200:
            cfg_name = "BASELINE configs[4] shape (per-GPU shard)"
        else:
            cfg_name = "custom shape"
        if a.config is not None:
            cfg_name = f"--config {a.config} = BASELINE configs[{a.config}]" + (f" ({cfg_name})" if "configs" not in cfg_name else "")
        if a.samples > 1:
            cfg_name += f", samples_num={a.samples} (images encoded once per step, embeddings re-used by every sample)"
        f_cap = caption_flops(L, K, I)
        bd = main_res["breakdown"]
        gemm_fl = sum(v["flops"] for k, v in bd.items() if k.startswith("gemm")) if bd else None
        out = dict(metric=metric_name(L, K, a.order, a.gamma, a.samples), value=round(value, 4), unit="captions/s",
                   n_gpus=world, steps=a.steps, warmup=a.warmup, ms_per_step=round(main_res["dt"] / a.steps * 1e3, 2),
                   higher_is_better=True, scaling="strong" if a.total_images is not None else "weak", vs_baseline=None,
                   dtype=DT[prec], data="synthetic",
                   config=dict(workload=f"{cfg_name}: " + (f"{n_total} random-pixel 224x224 images in total ({B} on rank 0)" if a.total_images is not None
                                                           else f"{B} random-pixel 224x224 images per GPU") + f", {a.order}, "
                                        f"L={L}, K={K}, I={I}, alpha=0.02 beta=2.0 tau=0.1, bert-base + CLIP ViT-B/32 shapes, "
                                        f"random-init weights (logit_scale {a.logit_scale}), synthetic vocab (1 CLIP token per word); "
                                        f"`value` = the {a.precision} engine at exp(logit_scale) = {np.exp(a.logit_scale):.1f}; "
                                        "`value_scale100` / `scale100_mode` (with --full) = the same workload, same steps and warm-up, through the engine the "
                                        "product path selects for the published checkpoints (logit scale 100)",
                               preset=a.config, samples_num=a.samples, images_per_gpu=B, total_images=n_total, sentence_len=L, candidate_k=K, num_iterations=I, order=a.order,
                               gamma=a.gamma, sentiment=a.sentiment if a.gamma is not None else None,
                               logit_scale=a.logit_scale, parallelism=f"image-sharded x{world} (no per-step collective); {main_res['streams']} concurrent "
                                           f"image sub-batches per GPU on separate HIP streams over one set of weights"
                                           + (f"; TEST RUN: {world} ranks share {torch.cuda.device_count()} device(s), {backend} rendezvous" if shared_gpu else "")),
                   ranks=dict(world_size=world, backend=("rccl (torch 'nccl')" if backend == "nccl" else backend) if world > 1 else None,
                              reported_by_backend=dist_world, devices_visible=torch.cuda.device_count(), shared_gpu=shared_gpu,
                              per_rank_images=[n for n, _ in main_res["per_rank"]],
                              per_rank_captions_per_s=[round(n * max(1, a.samples) * a.steps / d, 3) for n, d in main_res["per_rank"]],
                              host=main_res["host"], broadcast_s=main_res["broadcast_s"], gather_s=main_res["gather_s"]),
                   image_position_steps_per_s=round(value * L * I, 2),
                   algorithmic_tflop_per_caption=round(f_cap / 1e12, 3),
                   executed_tflop_per_caption=None if not gemm_fl else round(per_caption(gemm_fl, B, a.samples) / 1e12, 3),
                   roofline=roofline_of(main_res, prec),
                   kernel_ms_one_step={k: round(v["ms"], 1) for k, v in bd.items()},
                   kernel_ms_note="one extra untimed single-stream step with an event pair around every kernel class; the timed "
                                  "region only carries events around the roofline family",
                   clip_rows_per_step=st["clip_rows"] // max(1, a.steps), setup_s=round(main_res["setup_s"], 1),
                   dedup=dict(option="dedup=1 (default)" if not any(kv.replace(" ", "") == "dedup=0" for kv in a.opt) else "dedup=0",
                              candidate_seqs=st["clip_seqs"], deduplicated_seqs=st["dedup_seqs"],
                              note="exact de-duplication of identical candidate sentences (czc_dedup_stats): on these random-init towers "
                                   "softmax(logits / 0.1) is flat -- all K probabilities non-zero, no candidate masked to [PAD], no two "
                                   "decode to the same string -- so nothing is removed and `value` is unaffected; with a trained MLM head "
                                   "the zero-probability tail of the K candidates collapses to one caption "
                                   "(tests/test_step_gpu.py::test_dedup_is_exact: 25 % of the candidates, 20 % of the rows)"),
                   single_stream=None if main_res["single_ms"] is None else dict(
                       ms_per_step=round(main_res["single_ms"], 2), value=round(B * max(1, a.samples) / main_res["single_ms"] * 1e3, 4),
                       note="the same step on ONE engine / ONE stream (rank 0's images), wall-clock around the pass "
                            "`roofline.single_stream_pass` is measured on; `value` and `roofline.frac` come from the timed region"),
                   parity=dict(bar="fused score within 1e-3 of the reference's CPU path; identical argmax ids wherever the reference's own top-2 "
                                   "margin exceeds twice the engine's fused-score error",
                               bf16_engine="worst fused-score error 2.5e-4 on the full-size goldens; FREE-RUNNING it leaves the reference's "
                                           "trajectory only at near-ties (full-size goldens: 19 of 20 tokens on `full_senti`, reference margin "
                                           "2.7e-5 at the divergence; all other cases on it)",
                               scale100_engine="screen-then-refine: worst 2.8e-4 on the goldens (czc_step, 24 sample strata), ids identical to the all-split engine over "
                                               "25 600 image-steps of the fitted draw; on eleven more weight draws 2038 of 2048 images keep its ids over 10 "
                                               "sweeps, ten leave at near-ties of 2.3e-5 or less",
                               where="tests/test_step_gpu.py; profiles/r06_gpu_tests_summary.txt, profiles/r06_refine_validate_*.jsonl"),
                   batch_invariance=main_res["invariance"],
                   captions_crc32=None if main_res["ids_crc"] is None else dict(
                       value=main_res["ids_crc"], images=main_res["n_ids"],
                       note="crc32 of the final token ids of every image of the last timed step, gathered over the ranks in "
                            "image order: equal between an N-rank --total-images run and the 1-rank run of the same images"))
        if a.gamma is not None:
            def ctl_block(res, mode):
                v = n_total * a.steps * max(1, a.samples) / res["dt"]
                blk = dict(value=round(v, 4), unit="captions/s", ms_per_step=round(res["dt"] / a.steps * 1e3, 2), steps=a.steps, warmup=a.warmup)
                if mode == "exact":
                    blk["parity"] = ("the reference's sentence scorer on the decoded candidate strings: id for id on the *_ctx goldens "
                                     "(tests/test_control_gpu.py)")
                    blk["scorer"] = res["control"]
                else:
                    blk["parity"] = ("APPROXIMATE: a per-BERT-token table inside the bridge kernel (here a synthetic table); against a "
                                     "context-dependent tagger 29-50 % of the image-steps of the full-size *_ctx goldens pick another winner")
                return blk
            main_mode = "exact" if a.control == "exact" else "table"
            out["control_" + main_mode] = ctl_block(main_res, main_mode)
            if exact_res is not None:
                out["control_exact"] = ctl_block(exact_res, "exact")
            out["config"]["control"] = a.control
        if prec == native.PREC_REFINE:
            out["refine"] = refine_block(st)

        def alt_block(res, prec_, what):
            av = n_total * a.alt_steps * max(1, a.samples) / res["dt"]
            blk = dict(what=what, value=round(av, 4), unit="captions/s", dtype=DT[prec_], logit_scale=4.6052, steps=a.alt_steps,
                       warmup=a.alt_warmup, ms_per_step=round(res["dt"] / a.alt_steps * 1e3, 2), roofline=roofline_of(res, prec_),
                       single_stream_ms_per_step=None if res["single_ms"] is None else round(res["single_ms"], 2),
                       kernel_ms_one_step={k: round(v["ms"], 1) for k, v in res["breakdown"].items()})
            rs = res["stats"]
            if prec_ == native.PREC_REFINE:
                blk["refine"] = refine_block(rs)
            return blk

        if alt_res is not None:
            out["scale100_mode"] = alt_block(
                alt_res, native.PREC_REFINE,
                "same workload, SAME steps and warm-up as the headline leg, through the engine the product path selects for the published "
                "checkpoints (logit_scale = ln 100, clip/clip.py:95-98; conzic_amd.runtime.choose_precision): screen-then-refine "
                "-- all K candidates through the single-pass fp16 text tower, the candidates that carry the softmax_K mass "
                "re-encoded by the split-fp16 tower; fused score within 1e-3 on all K candidates and reference trajectories "
                "reproduced id for id (tests/test_step_gpu.py::test_step_parity_full_size_refine, "
                "::test_generate_free_running_full_size_refine)")
            out["value_scale100"] = out["scale100_mode"]["value"]
        if split_res is not None:
            out["scale100_all_split"] = alt_block(split_res, native.PREC_SPLIT,
                                                  "the same with every tower on split-fp16 MFMA (the round-2 product mode)")
        out["box_calibration"] = box_calibration() if a.full else None  # after the timed legs: it shares nothing with them
        if world == 1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(L, K, I, a.cpu_threads)
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    sys.stdout.flush()
    # the process ends through the interpreter (atexit handlers, library destructors): profilers and other tools that
    # record at process exit see the run; every engine was closed at the end of its leg


if __name__ == "__main__":
    main()
