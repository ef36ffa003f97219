"""The shared-prefix attention kernels of the CLIP-text tower, one launch at a time, row by row against fp64.

czc_test_attention_plan (tests/kernel_hooks.py: attention_plan) runs ONE launch on a host-given plan -- B trunk segments,
then B*K branch segments that see their image's trunk as key/value-only prefix -- through
  kernel 0: launch_attention with the prefix tables (attention_mfma_kernel, attention_mfma_split_kernel, attention_valu_kernel),
  kernel 1: the packed per-group kernels (attention_branch_kernel bf16 / fp16, attention_branch_split_kernel),
  kernel 2: the packed per-image kernel (attention_image_kernel, forced),
and tests/attn_ref.py states the same operation in numpy fp64 (held to the per-sequence formula by test_attn_ref_cpu.py).

 (a) geometry sweep on standard-normal data, bounds of the existing attention tests, every trunk and branch row;
 (b) leak: keys a query must NOT see are made overwhelmingly attractive (next candidate in the packed tile, own future key,
     another image's trunk); one leaked key replaces a victim's output by that key's v row;
 (c) spotlight: every query aligned with ONE allowed boundary key (trunk key 0, last trunk key, own key 0, diagonal): a
     dropped or shifted key loses > 0.99 of the weight;
 (d) kernels that may serve the same plan agree bit for bit (per-image == per-group; an image inside a batch == alone);
 (e) refusals and fall-backs are what the launcher says.
Every case prints its plan before launching (flushed), so a fault leaves the plan that was in flight in the log.
"""
import functools
import zlib

import numpy as np
import pytest

import attn_ref as R
import kernel_hooks as KH

pytestmark = pytest.mark.gpu

F32, BF16, SPLIT, FP16 = R.F32, R.BF16, R.SPLIT, R.FP16
SCALE = 0.125
# every (precision, kernel) pair that exists
PAIRS = [(F32, 0), (BF16, 0), (BF16, 1), (BF16, 2), (FP16, 0), (FP16, 1), (FP16, 2), (SPLIT, 0), (SPLIT, 1)]
PAIR_IDS = [f"{R.PREC_NAME[p]}-k{k}" for p, k in PAIRS]

# ---- the explicit edge table of (a) --------------------------------------------------------------------------------------------
# name, trunk_len per image, longest branch per image (branch lengths drawn per candidate from 1..that, one candidate holds it),
# K (a number, or relative to G = 32 // longest branch of image 0), heads, empty slots (own_len == 0: "first" / "inner" / "last"
# slot of the second group, or the whole "group"), img_max modes ("p" passed, "n" null)
EDGE = [
    # trunk 0 / 1 / 5 / 31 / 32; longest branch 1, 2, 3, 5, 8, 11, 16, 17, 32 -> G = 32, 16, 10, 6, 4, 2, 2, 1, 1
    ("t0_o1_G",        [0],          [1],         "G",    4,  None,    "p"),
    ("t1_o2_G+1",      [1],          [2],         "G+1",  8,  None,    "pn"),   # last group: one candidate
    ("t5_o3_G-1",      [5],          [3],         "G-1",  12, None,    "p"),    # 32 % 3 != 0
    ("t31_o1_K2",      [31],         [1],         2,      4,  None,    "pn"),   # 32 keys in all: the per-image kernel's limit
    ("t32_o5_K200",    [32],         [5],         200,    4,  None,    "p"),    # trunk of exactly one tile; 32 % 5 != 0, 200 % 6 != 0
    ("t5_o8_K1",       [5],          [8],         1,      8,  None,    "p"),
    ("t0_o11_G+1",     [0],          [11],        "G+1",  4,  None,    "p"),    # 32 % 11 != 0
    ("t1_o16_G",       [1],          [16],        "G",    12, None,    "n"),
    ("t5_o17_K2",      [5],          [17],        2,      4,  None,    "p"),    # G = 1
    ("t0_o32_K2",      [0],          [32],        2,      8,  None,    "p"),    # branches of exactly 32 rows
    ("t31_o1_K1024",   [31],         [1],         1024,   4,  None,    "p"),
    ("t5_o4_K512",     [5],          [4],         512,    4,  None,    "p"),
    ("t20_o3_K200",    [20],         [3],         200,    8,  None,    "n"),
    # trunks of two and three tiles (generic and per-group kernels; the per-image launcher falls back)
    ("t33_o5_G+1",     [33],         [5],         "G+1",  4,  None,    "p"),
    ("t45_o32_K2",     [45],         [32],        2,      8,  None,    "p"),    # 77 keys: the CLIP limit
    ("t64_o11_K200",   [64],         [11],        200,    4,  None,    "p"),
    ("t64_o13_G",      [64],         [13],        "G",    12, None,    "n"),    # 77 keys, three trunk tiles + own tile
    # three images whose longest branches differ inside one launch
    ("B3_o8_1_3",      [5, 31, 0],   [8, 1, 3],   "G+1",  4,  None,    "pn"),
    ("B3_o2_5_11",     [1, 20, 12],  [2, 5, 11],  200,    4,  None,    "pn"),
    ("B3_t32_33_64",   [32, 33, 64], [5, 11, 2],  7,      8,  None,    "pn"),
    ("B3_o16_17_32",   [0, 15, 5],   [16, 17, 32], 3,     12, None,    "pn"),
    # de-duplicated candidates (own_len == 0) at the first, an inner and the last slot of a group, and a whole group of them
    ("zero_first",     [5],          [4],         24,     4,  "first", "p"),
    ("zero_inner",     [31, 3],      [1, 4],      70,     8,  "inner", "pn"),
    ("zero_last",      [0],          [3],         31,     4,  "last",  "p"),
    ("zero_group",     [12],         [5],         20,     4,  "group", "pn"),
    ("zero_group0",    [0, 7],       [2, 2],      40,     4,  "group0", "p"),   # the FIRST group of image 0, no trunk in front of it
    # 2 heads: the generic and per-group launchers take them, the per-image one needs heads % 4 == 0 and falls back
    ("h2_t5_o3",       [5],          [3],         "G+1",  2,  None,    "p"),
    ("h2_B3",          [31, 0, 9],   [1, 6, 2],   9,      2,  "inner", "pn"),
]
# branches of 33..76 rows: generic kernels only, the packed launchers must refuse them
LONG = [
    ("long33",         [5],          [33],        3,      4,  None,    "p"),
    ("long50_t27",     [27],         [50],        4,      12, None,    "p"),
    ("long76_t1",      [1, 0],       [76, 40],    2,      8,  None,    "p"),
]
N_RANDOM = 10   # seeded random draws on top of the edge table (thin these, never the table, if the file gets slow)


class Plan:
    def __init__(self, name, trunk, own, heads, modes):
        self.name, self.heads, self.modes = name, heads, modes
        self.trunk = np.asarray(trunk, np.int32)
        self.own = np.asarray(own, np.int32)
        self.B, self.K = self.own.shape
        self.rows = int(self.trunk.sum() + self.own.sum())
        self.max_own = int(self.own.max())
        self.max_keys = int((self.trunk + self.own.max(1)).max())

    def __repr__(self):
        own = self.own.tolist() if self.own.size <= 96 else f"{self.own[:, :24].tolist()}... (first 24 of each image)"
        return f"plan {self.name}: B={self.B} K={self.K} heads={self.heads} trunk_len={self.trunk.tolist()} own_len={own}"

    def single(self, b):
        return Plan(f"{self.name}[image {b}]", self.trunk[b:b + 1], self.own[b:b + 1], self.heads, "p")

    def image_rows(self, b):
        toff, ooff, _ = R.plan_layout(self.trunk, self.own)
        return np.concatenate([np.arange(toff[b], toff[b] + self.trunk[b]),
                               np.arange(ooff[b, 0], ooff[b, 0] + self.own[b].sum())])


def _build(spec, seed):
    name, trunk, longest, K, heads, zeros, modes = spec
    rng = np.random.default_rng(seed)
    G = 32 // longest[0] if longest[0] <= 32 else 1
    K = {"G": G, "G-1": max(G - 1, 1), "G+1": G + 1}.get(K, K)
    own = np.stack([rng.integers(1, m + 1, size=K) for m in longest])
    for b, m in enumerate(longest):
        own[b, rng.integers(K)] = m
    if zeros:
        for b, m in enumerate(longest):
            Gb = 32 // m
            g0 = 0 if zeros == "group0" else min(1, (K - 1) // Gb) * Gb
            n = min(Gb, K - g0)
            sl = {"first": [g0], "inner": [g0 + n // 2], "last": [g0 + n - 1]}.get(zeros, list(range(g0, g0 + n)))
            own[b, sl] = 0
            if own[b].max() < m:   # keep the image's longest branch in place
                free = [k for k in range(K) if k not in sl]
                own[b, free[len(free) // 2]] = m
    return Plan(name, trunk, own, heads, modes)


def _random_specs():
    rng = np.random.default_rng(2024)
    out = []
    for i in range(N_RANDOM):
        B = int(rng.choice([1, 3]))
        longest = [int(x) for x in rng.choice([1, 2, 3, 5, 8, 11, 16, 17, 32], size=B)]
        trunk = [int(min(x, 77 - m)) for x, m in zip(rng.choice([0, 1, 5, 31, 32, 33, 45, 64], size=B), longest)]
        G = 32 // longest[0]
        K = int(rng.choice([1, 2, max(G - 1, 1), G, G + 1, 37]))
        heads = int(rng.choice([4, 8, 12]))
        zeros = [None, None, "first", "inner", "last", "group"][int(rng.integers(6))] if K > 2 else None
        out.append((f"random{i}", trunk, longest, K, heads, zeros, "pn"[int(rng.integers(2))]))
    return out


EDGE_PLANS = [_build(s, 10 + i) for i, s in enumerate(EDGE)]
LONG_PLANS = [_build(s, 50 + i) for i, s in enumerate(LONG)]
RANDOM_PLANS = [_build(s, 70 + i) for i, s in enumerate(_random_specs())]


def _serves(kernel, plan):
    """does the sweep run this plan through this kernel?  The per-image launcher is asked for every plan whose trunks fit its
    one trunk tile; where it cannot serve the plan (more than 32 keys, heads % 4 != 0) it falls back, which (e) pins down."""
    if kernel == 2:
        return int(plan.trunk.max()) <= 32
    return True


@functools.lru_cache(maxsize=None)
def _inputs(plan, kind):
    """fp32 host data [rows, 3, heads, 64] of a plan: "normal", a bait class of (b), or a spotlight class of (c)"""
    rng = np.random.default_rng(zlib.crc32(plan.name.encode()))
    if kind == "normal":
        return R.draw_qkv(rng, plan.rows, plan.heads), None, None
    x = R.draw_qkv(rng, plan.rows, plan.heads, R.V_SIGMA)
    if kind in R.SPOT_KINDS:
        return R.spotlight(x, plan.trunk, plan.own, kind)
    return R.bait(x, plan.trunk, plan.own, kind), None, None


@functools.lru_cache(maxsize=None)
def _reference(plan, kind, prec):
    """-> operands as the kernel reads them [rows, 3*Hd], fp64 reference, tolerance, rounding-model error"""
    x, tgt, trow = _inputs(plan, kind)
    xr = R.round_operand(prec, x.reshape(plan.rows, -1))
    if kind in R.SPOT_KINDS:
        ref, w = R.plan_ref(xr, plan.trunk, plan.own, plan.heads, SCALE, want_weight=tgt)
        assert w.min() > 0.99, (plan, kind, w.min())   # the construction: the target key carries the weight
    else:
        ref = R.plan_ref(xr, plan.trunk, plan.own, plan.heads, SCALE)
    if kind == "normal":
        return xr, ref, R.NORMAL_TOL[prec], 0.0
    tol, merr = R.rounding_tol(prec, xr, plan.trunk, plan.own, plan.heads, SCALE, ref)
    if prec in (BF16, FP16):   # beyond twice the standard-normal bound the construction would be too extreme
        assert tol <= 2 * R.NORMAL_TOL[prec], (plan, kind, tol, merr)
    return xr, ref, tol, merr


def _launch(prec, kernel, plan, xr, img_max, what):
    print(f"[{what} {R.PREC_NAME[prec]} kernel {kernel} img_max {'passed' if img_max else 'null'}] {plan!r}", flush=True)
    refused, out, guard = KH.attention_plan(prec, kernel, plan.trunk, plan.own, plan.heads, SCALE, xr, img_max=img_max)
    # no row outside the plan is written, whatever else happened
    assert np.all(guard == np.float32(KH.PLAN_SENTINEL[prec])), f"a guard row of the output was written: {plan!r}"
    return refused, out


def _assert_untouched(prec, out, plan):
    assert np.all(out == np.float32(KH.PLAN_SENTINEL[prec])), f"a refused launch wrote to the output: {plan!r}"


def _check(prec, kernel, plans, kind, what):
    """every plan through one (precision, kernel) pair against fp64; -> worst error / tolerance pair.  Reports the SMALLEST
    failing plan."""
    fails, worst = [], (0.0, 1.0, None)
    for plan in plans:
        if not _serves(kernel, plan):
            continue
        xr, ref, tol, _ = _reference(plan, kind, prec)
        for mode in plan.modes:
            refused, out = _launch(prec, kernel, plan, xr, mode == "p", f"{what}:{kind}")
            assert not refused, f"the launcher refused {plan!r}"
            assert np.isfinite(out).all(), f"non-finite output: {plan!r}"
            err = float(np.abs(out - ref).max()) if plan.rows else 0.0
            if err / tol > worst[0] / worst[1]:
                worst = (err, tol, plan.name)
            if not err < tol:
                bad = np.nonzero(np.abs(out - ref).max(1) >= tol)[0]
                img, cand, pos = R.plan_rows(plan.trunk, plan.own)
                fails.append((plan.rows, f"{plan!r} img_max {'passed' if mode == 'p' else 'null'}: max error {err:.3e} >= {tol:.3e} "
                                         f"on {bad.size} rows, first (image, candidate, position) "
                                         f"{[(int(img[r]), int(cand[r]), int(pos[r])) for r in bad[:6]]}"))
    print(f"[{what}:{kind}] {R.PREC_NAME[prec]} kernel {kernel}: worst error {worst[0]:.3e} at tolerance {worst[1]:.3e} ({worst[2]})", flush=True)
    assert not fails, f"{len(fails)} failing launches; the smallest: {min(fails)[1]}"
    return worst


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,kernel", PAIRS, ids=PAIR_IDS)
def test_geometry_sweep_against_fp64(prec, kernel):
    """standard-normal q, k, v over the edge table and the random draws: max abs error over EVERY trunk and branch row within
    the bound the same arithmetic is held to on plain sequences (f32 2e-5, bf16 1.5e-2, fp16 2e-3, split 3e-5); guard rows
    untouched, nothing non-finite.  Branches of 33..76 rows: generic kernels only, the packed launchers refuse them."""
    _check(prec, kernel, EDGE_PLANS + RANDOM_PLANS, "normal", "sweep")
    for plan in LONG_PLANS:
        xr, ref, tol, _ = _reference(plan, "normal", prec)
        refused, out = _launch(prec, kernel, plan, xr, True, "sweep:long")
        if kernel == 0:
            assert not refused and np.isfinite(out).all()
            err = float(np.abs(out - ref).max())
            assert err < tol, f"{plan!r}: {err:.3e} >= {tol:.3e}"
        else:
            assert refused, f"the packed launcher took a branch of more than 32 rows: {plan!r}"
            _assert_untouched(prec, out, plan)


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
def _leak_plans(kind):
    if kind == "other":   # the bait is the trunk of image 1
        return [p for p in EDGE_PLANS if p.B >= 2 and p.trunk[1] > 0]
    if kind == "next":
        return [p for p in EDGE_PLANS if p.K >= 2]
    return [p for p in EDGE_PLANS if p.max_own >= 2]


@pytest.mark.parametrize("kind", ["next", "future", "other"])
@pytest.mark.parametrize("prec,kernel", PAIRS, ids=PAIR_IDS)
def test_a_query_never_sees_a_key_it_must_not_see(prec, kernel, kind):
    """The forbidden keys of one class carry + 16 along head dimension 0 and their victims' queries 16 along it (32 in the
    logit, >= 25 above every allowed key): "next" the own keys of the odd candidates for the queries of the even ones (they
    share a packed tile), "future" a candidate's last own key for its earlier queries, "other" the trunk of image 1 for the
    queries of the other images.  The reference never sees the bait; a kernel that lets ONE through returns that key's v row
    (>= 50 tolerances away: test_attn_ref_cpu.py).  Tolerance: attn_ref.rounding_tol, computed here on the CPU."""
    _check(prec, kernel, _leak_plans(kind), kind, "leak")


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.SPOT_KINDS)
@pytest.mark.parametrize("prec,kernel", PAIRS, ids=PAIR_IDS)
def test_a_query_sees_every_boundary_key_it_must_see(prec, kernel, kind):
    """Every query is aligned with ONE allowed key of its own -- trunk key 0, the last trunk key (index 30, 31, 32, 44, 63 in
    the table), own key 0, the diagonal key -- so that the key carries > 0.99 of the softmax weight (asserted on the
    reference) and the context row is that key's v row: a dropped or shifted boundary key cannot average away."""
    _check(prec, kernel, EDGE_PLANS, kind, "spotlight")


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [BF16, FP16], ids=["bf16", "fp16"])
def test_per_image_and_per_group_kernels_agree_bitwise(prec):
    """The engine picks attention_image_kernel or attention_branch_kernel by batch size, and captions must not depend on the
    batch: on every plan both accept (heads % 4 == 0, at most 32 keys) they return the same bits."""
    n = 0
    for plan in EDGE_PLANS + RANDOM_PLANS:
        if plan.heads % 4 or plan.max_keys > 32:
            continue
        xr = _reference(plan, "normal", prec)[0]
        for mode in plan.modes:
            _, grp = _launch(prec, 1, plan, xr, mode == "p", "bitwise")
            _, img = _launch(prec, 2, plan, xr, mode == "p", "bitwise")
            np.testing.assert_array_equal(img, grp, err_msg=repr(plan))
            n += 1
    assert n >= 12


@pytest.mark.parametrize("prec,kernel", [(BF16, 1), (BF16, 2), (FP16, 1), (FP16, 2), (SPLIT, 1)],
                         ids=["bf16-k1", "bf16-k2", "fp16-k1", "fp16-k2", "split-fp16-k1"])
def test_an_image_does_not_depend_on_the_batch_it_is_launched_in(prec, kernel):
    """img_max passed: the rows of image b from a launch of three images == the same image launched alone, bit for bit (the
    packing factor is taken per image) -- test_attention_packing_does_not_couple_the_images_of_a_batch at kernel level."""
    n = 0
    for plan in EDGE_PLANS + RANDOM_PLANS:
        if plan.B < 2 or "p" not in plan.modes or not _serves(kernel, plan):
            continue
        xr = _reference(plan, "normal", prec)[0]
        _, full = _launch(prec, kernel, plan, xr, True, "batch")
        for b in range(plan.B):
            r = plan.image_rows(b)
            _, alone = _launch(prec, kernel, plan.single(b), xr[r], True, "alone")
            np.testing.assert_array_equal(full[r], alone, err_msg=f"image {b} of {plan!r}")
            n += 1
    assert n >= 9


# ---- (e) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,kernel", [(BF16, 1), (BF16, 2), (FP16, 1), (FP16, 2), (SPLIT, 1)],
                         ids=["bf16-k1", "bf16-k2", "fp16-k1", "fp16-k2", "split-fp16-k1"])
def test_the_packed_launchers_refuse_what_they_say_they_refuse(prec, kernel):
    """a branch of more than 32 rows, more than 96 keys, no branch row at all: status "refused", nothing written"""
    refused_plans = [Plan("max_own33", [5], [[3, 33, 1]], 4, "p"),
                     Plan("max_keys97", [70, 2], [[27, 5], [1, 1]], 4, "p"),
                     Plan("max_keys100_h12", [80], [[20] * 5], 12, "p"),
                     Plan("max_own0", [9, 4], [[0, 0, 0], [0, 0, 0]], 8, "p")]
    rng = np.random.default_rng(5)
    for plan in refused_plans:
        xr = rng.standard_normal((plan.rows, 3 * plan.heads * 64)).astype(np.float32)
        for img_max in (True, False):
            refused, out = _launch(prec, kernel, plan, xr, img_max, "refusal")
            assert refused, f"not refused: {plan!r}"
            _assert_untouched(prec, out, plan)
    # just inside: 96 keys and a branch of 32 rows are served (and right)
    plan = Plan("max_keys96", [64], [[32, 7, 1]], 4, "p")
    xr = R.round_operand(prec, rng.standard_normal((plan.rows, 3 * plan.heads * 64)).astype(np.float32))
    refused, out = _launch(prec, kernel, plan, xr, True, "refusal")
    assert not refused
    assert np.abs(out - R.plan_ref(xr, plan.trunk, plan.own, plan.heads, SCALE)).max() < R.NORMAL_TOL[prec]


@pytest.mark.parametrize("prec", [BF16, FP16], ids=["bf16", "fp16"])
def test_the_per_image_launcher_falls_back_to_the_per_group_kernel(prec):
    """per-image kernel requested with heads % 4 != 0 (2, 6 heads) or more than 32 keys: the launcher runs the per-group
    kernel -- same bits as kernel 1, not an error and not a silent third path"""
    plans = [p for p in EDGE_PLANS if p.heads % 4 or p.max_keys > 32]
    plans += [Plan("h6", [7], [[2, 3, 1, 3, 3, 2, 1, 1, 3, 2, 3]], 6, "p"), Plan("keys33", [31], [[2, 1, 2]], 4, "p"),
              Plan("trunk32", [32, 32], [[1, 1], [1, 1]], 4, "pn")]
    assert any(p.heads == 2 for p in plans) and any(int(p.trunk.max()) == 32 for p in plans)
    rng = np.random.default_rng(6)
    for plan in plans:
        xr = rng.standard_normal((plan.rows, 3 * plan.heads * 64)).astype(np.float32)
        for mode in plan.modes:
            _, grp = _launch(prec, 1, plan, xr, mode == "p", "fallback")
            _, img = _launch(prec, 2, plan, xr, mode == "p", "fallback")
            assert np.isfinite(grp).all()
            np.testing.assert_array_equal(img, grp, err_msg=repr(plan))
