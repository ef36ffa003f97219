"""The per-sequence attention kernels behind launch_attention, one launch at a time, row by row against fp64, in the forms the
BERT and vision towers run them: plain segments without a prefix, bidirectional or causal, own_off / own_len tables (with empty
segments) or the fixed_T form, max_keys tight or larger than the longest segment.

czc_test_attention_seq (tests/kernel_hooks.py: attention_seq) makes ONE launch_attention call; precision and the "mfma_attention"
switch select the kernel:
  f32 -> attention_valu_kernel<float>          bf16 -> attention_mfma_kernel<bf16_t>     fp16 -> attention_mfma_kernel<f16_t>
  split-fp16 -> attention_mfma_split_kernel    bf16, switch 0 -> attention_valu_kernel<bf16_t>
  split-fp16, switch 0 -> attention_valu_kernel<split_t>
and tests/attn_ref.py (seg_ref) states the operation in numpy fp64 (held to the per-sequence formula, and its one-key-wrong
mutants to their distances, by test_attn_ref_cpu.py).

 (a) sweep on standard-normal data, both mask modes, every layout: the bounds of the existing attention tests on EVERY row;
 (b) leak: the rows on either side of a victim segment are made overwhelmingly attractive; one leaked key replaces a victim's
     output by that key's v row (>= 20 / 200 / 10000 tolerances away in bf16 / fp16 / f32 and split-fp16);
 (c) spotlight: every query aligned with ONE key (key 0, the last visible key, either side of the 32-key tile edges, the
     diagonal) -- a dropped or shifted key loses > 0.99 of the weight -- and twin: key 0 and the last visible key share the
     weight, so a last key counted twice (an unmasked padding lane re-reads it) moves the row by >= 5 / 40 / 3000 tolerances;
 (d) launches that must not differ agree bit for bit (fixed_T form == tables; max_keys 96 == tight; a segment alone == in a batch);
 (e) refusals and the empty launch are what the launcher says.
Every case prints its layout before launching (flushed), so a fault leaves the layout that was in flight in the log.

Worst error / tolerance per pair, as measured on the MI355X (every test prints its own):
                      sweep (error at bound)      leak   spotlights (7 kinds)   twin
  f32-valu            0.08  (1.56e-6 / 2e-5)      0.05   < 0.01 (2.5e-8)        0.41
  bf16-mfma           0.88  (1.32e-2 / 1.5e-2)    0.16   < 0.01 (1.8e-8)        0.15
  bf16-valu           0.88  (1.32e-2 / 1.5e-2)    0.15   < 0.01 (1.8e-8)        0.14
  fp16-mfma           0.63  (1.26e-3 / 2e-3)      0.16   < 0.01 (1.7e-8)        0.15
  split-fp16-mfma     0.03  (9.6e-7 / 3e-5)       0.03   < 0.01 (7.0e-8)        0.14
  split-fp16-valu     0.06  (1.70e-6 / 3e-5)      0.03   < 0.01 (7.0e-8)        0.31
The VALU form of bf16, never measured before, sits inside the bf16 bound on standard-normal data: its worst row is the worst
row of the MFMA form (fixed_T = 15, 37 segments, causal), where the rounding of the output to bf16 dominates both.  On the
spotlights the context row is the target's v row, which the output type holds exactly.  Pointed at a seg_ref mutant in place of
the reference ("next" and "prev" for (b), "dup_last" for the twin), every pair fails on every layout that has such a key.
"""
import contextlib
import functools
import zlib

import numpy as np
import pytest

import attn_ref as R
import kernel_hooks as KH
from conzic_amd import native

pytestmark = pytest.mark.gpu

F32, BF16, SPLIT, FP16 = R.F32, R.BF16, R.SPLIT, R.FP16
SCALE = 0.125
# every (precision, "mfma_attention" switch) pair launch_attention has a kernel for
# (the two kernels of a precision side by side: they share a reference)
PAIRS = [(F32, 1), (BF16, 1), (BF16, 0), (FP16, 1), (SPLIT, 1), (SPLIT, 0)]
PAIR_IDS = ["f32-valu", "bf16-mfma", "bf16-valu", "fp16-mfma", "split-fp16-mfma", "split-fp16-valu"]
PAIR_NAME = dict(zip(PAIRS, PAIR_IDS))


class Layout:
    """segments back to back: `lens` rows each; fixed = every segment has T rows and the launch uses the fixed_T form"""

    def __init__(self, name, lens, heads, fixed=False):
        self.name, self.heads, self.fixed = name, int(heads), fixed
        self.lens = np.asarray(lens, np.int32).reshape(-1)
        self.n_seg = int(self.lens.size)
        self.rows = int(self.lens.sum())
        self.longest = int(self.lens.max()) if self.n_seg else 0
        self.live = int((self.lens > 0).sum())   # segments that have rows

    def __repr__(self):
        form = f"fixed_T={self.longest} n_seg={self.n_seg}" if self.fixed else f"lens={self.lens.tolist()}"
        return f"layout {self.name}: heads={self.heads} {form}"

    def single(self, s):
        return Layout(f"{self.name}[segment {s}]", self.lens[s:s + 1], self.heads)

    def as_table(self):
        return Layout(self.name + "[tables]", self.lens, self.heads)


MIXED = Layout("mixed_h8", [15, 1, 7, 16, 20, 77, 50, 64, 65, 2], 8)   # the lengths of test_attention_packed_sequences
TABLE = [
    Layout("one_row", [1], 4),
    Layout("ones70_h2", [1] * 70, 2),                # 70 work-groups of one query and one key
    Layout("tile_edge", [2, 31, 32, 33], 4),         # either side of one 32-key / 32-query tile
    Layout("two_tiles_h8", [63, 64, 65], 8),
    Layout("clip77_h12", [77, 1, 77], 12),
    Layout("three_tiles", [95, 96, 1, 96], 4),       # the full 3x3 tile grid
    MIXED,
    Layout("empty_inner", [5, 0, 33, 0, 0, 64, 0], 4),
    Layout("empty_ends", [0, 3, 0], 4),
] + [Layout(f"dead_waves_h{h}", [17, 50, 33], h) for h in (1, 3, 5, 6)]   # 3: a dead wave at 2 waves per group; 5, 6: at 4
FIXED = [Layout(f"fixed_n{n}_T{T}_h{h}", [T] * n, h, fixed=True)
         for T, h in ((1, 4), (15, 4), (32, 4), (33, 4), (96, 4), (50, 12), (64, 12)) for n in (1, 3, 37)]
N_RANDOM = 8


def _random_layouts():
    rng = np.random.default_rng(2025)
    out = []
    for i in range(N_RANDOM):
        lens = rng.integers(0, 97, size=int(rng.integers(1, 9)))
        if lens.max() == 0:
            lens[0] = 1
        out.append(Layout(f"random{i}", lens, int(rng.choice([1, 2, 3, 4, 6, 8, 12]))))
    return out


RANDOM = _random_layouts()
EDGE = TABLE + FIXED
SPOT_KINDS = R.SEG_SPOT_KINDS + ("twin",)


@contextlib.contextmanager
def _switch(mfma):
    """the "mfma_attention" switch for the launches inside, the default (1) after them"""
    lib = native.load_test()
    try:
        assert lib.czc_test_set_option(b"mfma_attention", int(mfma)) == 0
        yield
    finally:
        lib.czc_test_set_option(b"mfma_attention", 1)


def _inputs(lay, kind, causal):
    """fp32 host data [rows, 3, heads, 64]: "normal", "bait0" / "bait1" of (b), a spotlight kind or "twin" of (c).  -> x, targets"""
    rng = np.random.default_rng(zlib.crc32(lay.name.encode()))
    if kind == "normal":
        return R.draw_qkv(rng, lay.rows, lay.heads), None
    x = R.draw_qkv(rng, lay.rows, lay.heads, R.V_SIGMA)
    if kind == "twin":
        return R.seg_twin(x, lay.lens, causal)
    if kind in R.SEG_SPOT_KINDS:
        return R.seg_spotlight(x, lay.lens, kind, causal)[:2]
    return R.seg_bait(x, lay.lens, {"bait0": 0, "bait1": 1}[kind]), None


@functools.lru_cache(maxsize=160)   # one pass over every layout in both mask modes; the bf16 / split pairs of a kind share it
def _reference(lay, kind, causal, prec):
    """-> operands as the kernel reads them [rows, 3*Hd], fp64 reference, tolerance"""
    x, tgt = _inputs(lay, kind, causal)
    xr = R.round_operand(prec, x.reshape(lay.rows, -1))
    if tgt is not None:
        ref, w = R.seg_ref(xr, lay.lens, lay.heads, causal, SCALE, want_weight=tgt)
        assert w.min() > 0.99, (lay, kind, causal, w.min())   # the construction: the target key(s) carry the weight
    else:
        ref = R.seg_ref(xr, lay.lens, lay.heads, causal, SCALE)
    if kind == "normal":
        return xr, ref, R.NORMAL_TOL[prec]
    tol, merr = R.seg_rounding_tol(prec, xr, lay.lens, lay.heads, causal, SCALE, ref)
    if prec in (BF16, FP16):   # beyond twice the standard-normal bound the construction would be too extreme
        assert tol <= 2 * R.NORMAL_TOL[prec], (lay, kind, causal, tol, merr)
    return xr, ref, tol


def _launch(prec, lay, xr, causal, what, max_keys=0):
    print(f"[{what} {R.PREC_NAME[prec]} causal {causal} max_keys {max_keys or 'tight'}] {lay!r}", flush=True)
    if lay.fixed:
        out, guard = KH.attention_seq(prec, xr, lay.heads, causal, SCALE, n_seg=lay.n_seg, fixed_T=lay.longest, max_keys=max_keys)
    else:
        out, guard = KH.attention_seq(prec, xr, lay.heads, causal, SCALE, seq_len=lay.lens, max_keys=max_keys)
    # no row outside the segments is written, whatever else happened (rows of empty segments do not exist)
    assert np.all(guard == np.float32(KH.PLAN_SENTINEL[prec])), f"a guard row of the output was written: {lay!r}"
    assert out.shape == (lay.rows, lay.heads * 64)
    return out


def _check(prec, mfma, layouts, kind, what):
    """every layout in both mask modes through one (precision, kernel) pair against fp64; -> worst (error, tolerance, where).
    Reports the SMALLEST failing layout and its first failing (segment, position, head)."""
    fails, worst = [], (0.0, 1.0, None)
    with _switch(mfma):
        for lay in layouts:
            for causal in (0, 1):
                xr, ref, tol = _reference(lay, kind, causal, prec)
                out = _launch(prec, lay, xr, causal, f"{what}:{kind}")
                assert np.isfinite(out).all(), f"non-finite output: {lay!r} causal {causal}"
                diff = np.abs(out - ref)
                err = float(diff.max()) if lay.rows else 0.0
                if err / tol > worst[0] / worst[1]:
                    worst = (err, tol, f"{lay.name} causal {causal}")
                if not err < tol:
                    seg, pos, _ = R.seg_rows(lay.lens)
                    bad = np.argwhere(diff.reshape(lay.rows, lay.heads, 64).max(-1) >= tol)
                    fails.append((lay.rows, f"{lay!r} causal {causal}: max error {err:.3e} >= {tol:.3e} on {np.unique(bad[:, 0]).size} rows, "
                                            f"first (segment, position, head) {[(int(seg[r]), int(pos[r]), int(h)) for r, h in bad[:6]]}"))
    print(f"[{what}:{kind}] {PAIR_NAME[(prec, mfma)]}: worst error {worst[0]:.3e} at tolerance {worst[1]:.3e} = {worst[0] / worst[1]:.2f} "
          f"({worst[2]})", flush=True)
    assert not fails, f"{len(fails)} failing launches; the smallest: {min(fails)[1]}"
    return worst


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,mfma", PAIRS, ids=PAIR_IDS)
def test_layout_sweep_against_fp64(prec, mfma):
    """standard-normal q, k, v over the table, the fixed_T forms and the random draws, both mask modes: max abs error over EVERY
    row within the bound the same arithmetic is held to by the existing attention tests (f32 2e-5, bf16 1.5e-2 -- the VALU form
    of bf16 too --, fp16 2e-3, split 3e-5); guard rows untouched, nothing non-finite."""
    _check(prec, mfma, EDGE + RANDOM, "normal", "sweep")


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,mfma", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("parity", [0, 1])
def test_a_query_never_sees_a_key_of_a_neighbouring_segment(prec, mfma, parity):
    """The keys of every second segment carry + 16 along head dimension 0 and the queries of the segments between them 16 along
    it (32 in the logit, >= 25 above every allowed key): the row behind a victim segment's last key and the row in front of its
    first are bait.  The reference never sees them; a kernel that lets ONE through returns that key's v row, at least 20 (bf16),
    200 (fp16), 10000 (f32, split-fp16) tolerances away (test_attn_ref_cpu.py).  Under the bidirectional mask nothing but the
    `key < nk` test of the padding lanes keeps the following row out.  Tolerance: attn_ref.seg_rounding_tol, from the CPU."""
    _check(prec, mfma, [lay for lay in EDGE if lay.live >= 2], f"bait{parity}", "leak")


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,mfma", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("kind", SPOT_KINDS)
def test_a_query_sees_every_key_it_must_see_once(prec, mfma, kind):
    """Spotlights: every query aligned with ONE key of its own -- key 0, the last visible key, the keys at 31, 32, 63, 64
    (clamped to the last visible key), the diagonal -- which then carries > 0.99 of the weight (asserted on the reference
    before the launch): a dropped or shifted key cannot average away.  Twin: key 0 and the last visible key carry half of the
    weight each; a padding lane that re-reads the clamped last key and is not masked counts it twice and moves the row by a
    sixth of v_last - v_0, at least 5 (bf16), 40 (fp16), 3000 (f32, split-fp16) tolerances (test_attn_ref_cpu.py)."""
    _check(prec, mfma, EDGE, kind, "spotlight")


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,mfma", PAIRS, ids=PAIR_IDS)
def test_the_fixed_length_form_equals_the_table_form_bitwise(prec, mfma):
    """SegTable with own_len null (segment s = rows s*T .. s*T+T-1) against tables that say the same"""
    with _switch(mfma):
        for lay in FIXED:
            for causal in (0, 1):
                xr = _reference(lay, "normal", causal, prec)[0]
                fixed = _launch(prec, lay, xr, causal, "fixed")
                table = _launch(prec, lay.as_table(), xr, causal, "table")
                np.testing.assert_array_equal(fixed, table, err_msg=f"{lay!r} causal {causal}")


@pytest.mark.parametrize("prec,mfma", PAIRS, ids=PAIR_IDS)
def test_a_larger_max_keys_changes_no_bit(prec, mfma):
    """The ragged BERT path passes the longest segment of the whole run, not of the launch: max_keys sizes the row stride of
    the V^T / K^T tiles in shared memory (and with it how many heads share a work-group) and nothing else."""
    with _switch(mfma):
        for lay in EDGE + RANDOM:
            for causal in (0, 1):
                xr = _reference(lay, "normal", causal, prec)[0]
                tight = _launch(prec, lay, xr, causal, "max_keys")
                wide = _launch(prec, lay, xr, causal, "max_keys", max_keys=96)
                np.testing.assert_array_equal(wide, tight, err_msg=f"{lay!r} causal {causal}")


@pytest.mark.parametrize("prec,mfma", PAIRS, ids=PAIR_IDS)
def test_a_segment_does_not_depend_on_the_batch_it_is_launched_in(prec, mfma):
    """each segment of the mixed layout launched alone == its rows in the launch of all ten, bit for bit"""
    off = np.concatenate([[0], np.cumsum(MIXED.lens)])
    with _switch(mfma):
        for causal in (0, 1):
            xr = _reference(MIXED, "normal", causal, prec)[0]
            full = _launch(prec, MIXED, xr, causal, "batch")
            for s in range(MIXED.n_seg):
                r = slice(int(off[s]), int(off[s + 1]))
                alone = _launch(prec, MIXED.single(s), xr[r], causal, "alone")
                np.testing.assert_array_equal(full[r], alone, err_msg=f"segment {s} of {MIXED!r} causal {causal}")


# ---- (e) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,mfma", PAIRS, ids=PAIR_IDS)
def test_the_launcher_refuses_more_than_96_keys(prec, mfma):
    """max_keys 97 over short segments, a table whose longest segment has 97 rows, the fixed_T form at T = 97: the launcher's
    own error, for every kernel family.  96 is served (the sweep).  A max_keys below the longest segment never reaches the
    launcher: the kernels would trust it."""
    rng = np.random.default_rng(9)
    cases = [(Layout("keys97_passed", [5, 3], 4), 97), (Layout("seg97", [97, 3], 4), 0), (Layout("fixed97", [97] * 2, 4, fixed=True), 0)]
    with _switch(mfma):
        for lay, max_keys in cases:
            xr = rng.standard_normal((lay.rows, 3 * lay.heads * 64)).astype(np.float32)
            for causal in (0, 1):
                with pytest.raises(native.NativeError, match="97 keys per segment unsupported"):
                    _launch(prec, lay, xr, causal, "refusal", max_keys=max_keys)
        lay = Layout("keys_below_longest", [5, 40], 4)
        xr = rng.standard_normal((lay.rows, 3 * lay.heads * 64)).astype(np.float32)
        with pytest.raises(native.NativeError, match="below the longest segment") as e:
            _launch(prec, lay, xr, 0, "refusal", max_keys=39)
        assert e.value.code == native.ERR_ARG


@pytest.mark.parametrize("prec,mfma", PAIRS, ids=PAIR_IDS)
def test_an_empty_launch_succeeds_and_writes_nothing(prec, mfma):
    """n_seg = 0 in both forms: status 0, every byte of the output buffer still at its pre-fill"""
    with _switch(mfma):
        for lay in (Layout("no_segments", [], 4), Layout("no_segments_fixed", [], 4, fixed=True)):
            for causal in (0, 1):
                out = _launch(prec, lay, np.zeros((0, 3 * lay.heads * 64), np.float32), causal, "empty")   # asserts the guard rows
                assert out.shape == (0, lay.heads * 64)
