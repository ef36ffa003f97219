"""The row and embedding kernels of csrc/rowops.hip and csrc/ragged.hip, one launcher at a time, against the host references of
tests/rowops_ref.py: float64 with a derived forward-error bound where the result is rounded arithmetic, bit for bit where it is a single
IEEE add, a storage rounding or the promise that two kernels state the same arithmetic.  Every output sits between guard words.

Measured on the MI355X, worst |error| / bound over all rows of all cases (the fp32 bound is a worst-case one, so a correct kernel sits
well below 1; a typed output's bound is dominated by half a unit in the last place of the storage type, which rounding does reach):
  launch_layernorm:  fp32 output 0.19 (the kernels of all four precisions);  typed output bf16 0.995, fp16 0.992, split hi + lo 0.20;
  launch_layernorm_x16 with row_idx:  bf16 0.985, fp16 0.982;
  launch_bert_embed:  fp32 output 0.18;  typed bf16 0.99, fp16 0.99, split 0.19;
  clip_embed statistics of the stored fp16 row (mean, rstd):  H = 64: 0.00, 0.14;  H = 512: 0.09, 0.17;  H = 768: 0.06, 0.11;
  launch_l2_normalize:  0.29;
  launch_ln_finalize:  see test_ln_finalize_against_fp64_of_the_same_partials.
"""
import numpy as np
import pytest

import kernel_hooks as KH
import rowops_ref as RR
from rowops_ref import BF16, F16, F16X3, F32

pytestmark = pytest.mark.gpu

PRECS = (F32, BF16, F16, F16X3)
NAME = {F32: "f32", BF16: "bf16", F16: "fp16", F16X3: "split"}
RATIO = {}   # what the module docstring quotes: label -> worst error / bound seen in this run


def _note(label, r):
    RATIO[label] = max(RATIO.get(label, 0.0), float(r))


def _check(y, y64, tol, label, what):
    r = RR.worst_ratio(y, y64, tol)
    _note(label, r)
    print(f"[ratio] {label}: {r:.3f}   ({what})")
    assert RR.inside(y, y64, tol).all(), (label, what, r)


def _untouched(g):
    g.assert_guards()
    return all(KH.untouched(v).all() for v in g.values())


def _typed_ok(prec, H):
    return not (prec == F16X3 and H % 8)   # split rows are whole groups of 8 elements: the launchers refuse the typed output


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("H", RR.LN_H)
def test_layernorm_rows(prec, H):
    """launch_layernorm: fp32 and typed outputs of one launch, M = 1 / 4 / 5 / 37 rows (four rows per work-group), both eps, ordinary
    rows, rows of mean 30 and spread 0.1, a constant row (y == beta bit for bit), the in-place form, and 37 picks with repeats out of 50
    source rows through row_idx."""
    x, g, b, idx = RR.ln_inputs(H)
    typed = _typed_ok(prec, H)
    mode = 3 if typed else 2
    for eps in RR.LN_EPS:
        for M in RR.LN_M:
            xs = x[:M]
            if not typed:
                ref, out = KH.layernorm_rows(prec, xs, g, b, eps, mode=3)
                assert ref and _untouched(out)
            ref, out = KH.layernorm_rows(prec, xs, g, b, eps, mode=mode)
            assert not ref
            out.assert_guards()
            y32 = out["y_f32"].reshape(M, H)
            y64, tol = RR.layernorm_bound(xs, g, b, eps)
            _check(y32, y64, tol, f"layernorm f32-out ({NAME[prec]} kernel)", f"prec {NAME[prec]} H {H} M {M} eps {eps}")
            if M > 2:
                assert np.array_equal(y32[2].view(np.uint32), b.view(np.uint32)), "constant row: y must be beta"
            if typed:
                st = KH.Stored(prec, out["y_act"], M * H)
                assert RR.bits_equal(st.bits, RR.store_bits(prec, y32)), "typed output is the storage rounding of the fp32 output"
                y64t, tolt = RR.layernorm_bound(xs, g, b, eps, prec=prec)
                _check(st.f32.reshape(M, H), y64t, tolt, f"layernorm {NAME[prec]}-out", f"H {H} M {M} eps {eps}")
            # the in-place form of the vision pre-LN: y_f32 == x
            ref, al = KH.layernorm_rows(prec, xs, g, b, eps, mode=mode | 4)
            assert not ref
            al.assert_guards()
            assert np.array_equal(al["y_f32"].view(np.uint32), out["y_f32"].view(np.uint32))
            assert np.array_equal(al["y_act"].view(np.uint32), out["y_act"].view(np.uint32))
        # row_idx: the CLIP pooling and the vision post-LN
        ref, full = KH.layernorm_rows(prec, x, g, b, eps, mode=mode)
        ref2, pick = KH.layernorm_rows(prec, x, g, b, eps, row_idx=idx, mode=mode)
        assert not ref and not ref2
        full.assert_guards(), pick.assert_guards()
        yp = pick["y_f32"].reshape(idx.size, H)
        y64, tol = RR.layernorm_bound(x, g, b, eps, idx)
        _check(yp, y64, tol, f"layernorm f32-out ({NAME[prec]} kernel)", f"prec {NAME[prec]} H {H} row_idx eps {eps}")
        assert np.array_equal(yp.view(np.uint32), full["y_f32"].reshape(-1, H)[idx].view(np.uint32))
        if typed:
            sp, sf = KH.Stored(prec, pick["y_act"], idx.size * H), KH.Stored(prec, full["y_act"], RR.N_SRC * H)
            assert np.array_equal(sp.f32.reshape(-1, H).view(np.uint32), sf.f32.reshape(-1, H)[idx].view(np.uint32))
            assert RR.bits_equal(sp.bits, RR.store_bits(prec, yp))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("H", [6, 1028])
def test_layernorm_refuses_widths_it_cannot_serve(prec, H):
    x = np.ones((5, H), np.float32)
    ref, out = KH.layernorm_rows(prec, x, np.ones(H), np.zeros(H), 1e-5, mode=2 if prec == F16X3 and H % 8 else 3)
    assert ref and _untouched(out)


@pytest.mark.parametrize("prec", [BF16, F16])
def test_layernorm_of_fp16_rows_with_row_idx(prec):
    x, g, b, idx = RR.ln_inputs(512)
    xr = x.astype(np.float16).astype(np.float32)
    for eps in RR.LN_EPS:
        ref, out = KH.layernorm_x16_rows(prec, x, g, b, eps, row_idx=idx)
        assert not ref
        out.assert_guards()
        st = KH.Stored(prec, out["y_act"], idx.size * 512)
        y64, tol = RR.layernorm_bound(xr, g, b, eps, idx, prec=prec)
        _check(st.f32.reshape(-1, 512), y64, tol, f"layernorm_x16 {NAME[prec]}", f"row_idx eps {eps}")
        _, full = KH.layernorm_x16_rows(prec, x, g, b, eps)
        sf = KH.Stored(prec, full["y_act"], RR.N_SRC * 512)
        assert np.array_equal(st.bits.reshape(-1, 512), sf.bits.reshape(-1, 512)[idx])
        assert np.array_equal(sf.f32.reshape(-1, 512), KH.layernorm_x16(prec, x, g, b, eps))
    ref, out = KH.layernorm_x16_rows(prec, x[:, :256], g[:256], b[:256], 1e-5)
    assert ref and _untouched(out)
    ref, out = KH.layernorm_x16_rows(F32, x, g, b, 1e-5)
    assert ref and _untouched(out)


@pytest.mark.parametrize("prec", [F32, F16X3])
@pytest.mark.parametrize("H", [320, 768])
def test_layernorm_of_split_k_slabs_is_the_reduce_then_layernorm(prec, H):
    """launch_layernorm_splitk: the float32 sum of the slabs in slab order, then bias, then the residual, normalised: bit for bit what
    launch_layernorm gives on that sum."""
    rng = np.random.default_rng(H)
    g = (1 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal(H)).astype(np.float32)
    for nslab in (1, 2, 4):
        for M in (5, 37):
            slabs = rng.standard_normal((nslab, M, H + 8)).astype(np.float32)
            bias = rng.standard_normal(H).astype(np.float32)
            resid = (rng.standard_normal((M, H + 4)) * 2).astype(np.float32)
            for use_bias in (False, True):
                for use_resid in (False, True):
                    v = slabs[0, :, :H].copy()
                    for z in range(1, nslab):
                        v = v + slabs[z, :, :H]
                    if use_bias:
                        v = v + bias
                    if use_resid:
                        v = v + resid[:, :H]
                    assert v.dtype == np.float32
                    ref, out = KH.layernorm_splitk(prec, slabs, H, bias if use_bias else None, resid if use_resid else None, g, b, 1e-12)
                    ref2, exp = KH.layernorm_rows(prec, v, g, b, 1e-12, mode=3)
                    assert not ref and not ref2
                    out.assert_guards(), exp.assert_guards()
                    assert np.array_equal(out["y_f32"].view(np.uint32), exp["y_f32"].view(np.uint32)), (nslab, M, use_bias, use_resid)
                    assert np.array_equal(out["y_act"].view(np.uint32), exp["y_act"].view(np.uint32)), (nslab, M, use_bias, use_resid)
    for bad in (BF16, F16):
        ref, out = KH.layernorm_splitk(bad, slabs, H, None, None, g, b, 1e-12)
        assert ref and _untouched(out)


@pytest.mark.parametrize("M", [1, 255, 257])
def test_ln_finalize_against_fp64_of_the_same_partials(M):
    """ln_finalize_kernel forms var = E[x^2] - mean^2 in fp32 from 16 partials summed in order.  Against fp64 of the same partials, with
    the bound of tests/rowops_ref.py (relative rstd error ~ u (1 + mean^2 / var)), rows of fp16 values whose mean / spread ratio is 0, 1,
    4 and 16.  Measured on the MI355X (M = 257, eps = 1e-5), worst |error| / bound per mean / spread ratio, (mean, rstd):
        ratio 0: (0.04, 0.19);  ratio 1: (0.14, 0.07);  ratio 4: (0.00, 0.06);  ratio 16: (0.00, 0.06)
    (the sums of these fp16 values are exact in fp32 from ratio 4 on) and the worst relative rstd error itself: 1.3e-7, 1.6e-7 (2.1e-7
    at M = 255), 1.5e-6, 2.3e-5.  Every case is inside the bound, which grows with 1 + mean^2 / var as the error does: at |mean| = 16
    spreads the subtraction costs about 400 ulps of rstd (two of fp32's seven digits; still 20 times finer than the fp16 operands it
    scales), so the "few ulps, not digits" of the kernel's comment holds for rows whose |mean| is of the order of their spread, as the
    comment assumes, and no further."""
    eps = 1e-5
    _, ratio, part = RR.lnf_inputs(M, M + 3)
    ref, out = KH.ln_finalize(part, M, eps)
    assert not ref
    out.assert_guards()
    stat = out["stat"].reshape(M, 2)
    m64, r64, dm, rho = RR.ln_finalize_bound(part, M, eps)
    em, er = np.abs(stat[:, 0] - m64), np.abs(stat[:, 1] / r64 - 1)
    for q in RR.LNF_RATIOS:
        s = ratio == q
        if s.any():
            print(f"[ratio] ln_finalize M {M} mean/spread {q:g}: mean {float((em[s] / dm[s]).max()):.3f} rstd {float((er[s] / rho[s]).max()):.3f}"
                  f"   worst relative rstd error {float(er[s].max()):.2e}")
    assert (em <= dm).all(), float((em / dm).max())
    assert (er <= rho).all(), float((er / rho).max())


# ---- embeddings --------------------------------------------------------------------------------------------------------------------------
def _bert_tables(H, V=50, n_pos=8, seed=0):
    rng = np.random.default_rng(H + seed)
    word = (rng.standard_normal((V, H)) * 0.5).astype(np.float32)
    pos = (rng.standard_normal((n_pos, H)) * 0.1).astype(np.float32)
    typ = (rng.standard_normal(H) * 0.1).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal(H)).astype(np.float32)
    return word, pos, typ, g, b


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("H", [64, 768])
def test_bert_embed(prec, H):
    """(word[id] + type0) + pos[t] in float32, then launch_layernorm's arithmetic: bit for bit the LayerNorm kernel on those rows."""
    V, B, T, eps = 50, 3, 5, 1e-12
    word, pos, typ, g, b = _bert_tables(H)
    ids = np.random.default_rng(1).integers(0, V, (B, T)).astype(np.int32)
    ids[0, 0], ids[2, 4], ids[1, 2] = 0, V - 1, V - 1
    rows = RR.bert_embed_rows(ids, np.tile(np.arange(T), B), word, pos, typ)
    ref, out = KH.bert_embed(prec, ids, word, pos, typ, g, b, eps)
    ref2, exp = KH.layernorm_rows(prec, rows, g, b, eps, mode=3)
    assert not ref and not ref2
    out.assert_guards()
    assert np.array_equal(out["y_f32"].view(np.uint32), exp["y_f32"].view(np.uint32))
    assert np.array_equal(out["y_act"].view(np.uint32), exp["y_act"].view(np.uint32))
    y64, tol = RR.layernorm_bound(rows, g, b, eps)
    _check(out["y_f32"].reshape(B * T, H), y64, tol, "bert_embed f32-out", f"prec {NAME[prec]} H {H}")
    y64, tol = RR.layernorm_bound(rows, g, b, eps, prec=prec)
    _check(KH.Stored(prec, out["y_act"], B * T * H).f32.reshape(B * T, H), y64, tol, f"bert_embed {NAME[prec]}-out", f"H {H}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("H", [64, 768])
def test_bert_embed_ragged(prec, H):
    """Packed ragged rows: each equals the dense kernel's row of the same (id, position) bit for bit; the padding columns hold a valid id
    whose embedding row is 1e30 and are never read; rows behind the packed range keep the pattern."""
    V, eps = 50, 1e-12
    word, pos, typ, g, b = _bert_tables(H)
    poison = 17
    word[poison] = 1e30
    row_len = np.array([5, 1, 3, 2], np.int32)
    row_off = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int32)
    rng = np.random.default_rng(2)
    ids = rng.integers(0, V, (4, 7)).astype(np.int32)
    ids[ids == poison] = 3
    ids[0, 0], ids[3, 1] = 0, V - 1
    dense_ids = ids[:, :5].copy()
    n_rows = int(row_off[-1])
    for run in (None, np.array([2, 0, 3, 1], np.int32)):
        src = np.arange(4) if run is None else run
        padded = ids.copy()
        for i in range(4):   # sequence i reads id row src[i]: behind its own length that row holds the poison
            padded[src[i], row_len[i]:] = poison
        ref, out = KH.bert_embed_ragged(prec, padded, run, row_off, row_len, 5, n_rows + 2, word, pos, typ, g, b, eps)
        ref2, dense = KH.bert_embed(prec, dense_ids, word, pos, typ, g, b, eps)
        assert not ref and not ref2
        out.assert_guards()
        yf, df = out["y_f32"].reshape(n_rows + 2, H), dense["y_f32"].reshape(4, 5, H)
        ya, da = out["y_act"].view(np.uint32).reshape(n_rows + 2, -1), dense["y_act"].view(np.uint32).reshape(4, 5, -1)
        for i in range(4):
            for t in range(row_len[i]):
                assert np.array_equal(yf[row_off[i] + t].view(np.uint32), df[src[i], t].view(np.uint32)), (i, t)
                if H % 8 == 0 or prec != F16X3:
                    assert np.array_equal(ya[row_off[i] + t], da[src[i], t]), (i, t)
        assert np.isfinite(yf[:n_rows]).all() and np.abs(yf[:n_rows]).max() < 100
        assert KH.untouched(yf[n_rows:]).all() and KH.untouched(ya[n_rows:]).all()
    ref, out = KH.bert_embed_ragged(prec, ids[:, :4], None, row_off, np.minimum(row_len, 4), 5, n_rows + 2, word, pos, typ, g, b, eps)
    assert ref and _untouched(out)   # max_T > ids_stride


@pytest.mark.parametrize("prec", PRECS)
def test_embed_launchers_refuse_widths_they_cannot_serve(prec):
    for H in (6, 1028):
        word, pos, typ, g, b = _bert_tables(H, V=4, n_pos=4)
        ids = np.array([[0, 3, 1]], np.int32)
        ref, out = KH.bert_embed(prec, ids, word, pos, typ, g, b, 1e-12)
        assert ref and _untouched(out)
        ref, out = KH.bert_embed_ragged(prec, ids, None, [0, 3], [3], 3, 3, word, pos, typ, g, b, 1e-12)
        assert ref and _untouched(out)
    if prec == F16X3:   # split rows are whole groups of 8 elements
        word, pos, typ, g, b = _bert_tables(68, V=4, n_pos=4)
        ref, out = KH.bert_embed(prec, np.array([[0, 3, 1]], np.int32), word, pos, typ, g, b, 1e-12)
        assert ref and _untouched(out)


def _clip_plan():
    """2 trunks + 2 x 3 branches over 6 id rows: trunk b reads id row 3 b from position 0, branch (b, k) id row 3 b + k from the trunk's
    length on; a de-duplicated branch (own_len 0), one-row branches, packed rows back to back"""
    own_len = np.array([3, 2, 4, 0, 1, 5, 1, 0], np.int32)
    seg_src = np.array([0, 3, 0, 1, 2, 3, 4, 5], np.int32)
    seg_pos0 = np.array([0, 0, 3, 3, 3, 2, 2, 2], np.int32)
    own_off = np.concatenate([[0], np.cumsum(own_len)[:-1]]).astype(np.int32)
    return own_len, seg_src, seg_pos0, own_off, int(own_len.sum())


@pytest.mark.parametrize("H", [64, 512, 768])
def test_clip_embed(H):
    """fp32: tok[id] + pos[p] bit for bit; fp16 rows: that sum rounded once; stat: (mean, rstd) of the STORED fp16 row against fp64
    within the two-pass bound.  Rows of no segment keep the pattern."""
    V, stride, eps = 40, 20, 1e-5
    rng = np.random.default_rng(H)
    tok = (rng.standard_normal((V, H)) * 0.5 + 0.3).astype(np.float32)
    pos = (rng.standard_normal((stride, H)) * 0.1).astype(np.float32)
    ids = rng.integers(0, V, (6, stride)).astype(np.int32)
    ids[0, 0], ids[4, 2] = 0, V - 1
    own_len, seg_src, seg_pos0, own_off, n = _clip_plan()
    x32, written = RR.clip_embed_rows(ids, seg_src, seg_pos0, own_off, own_len, tok, pos, n + 2)
    assert written[:n].all() and not written[n:].any()
    for mode in (0, 1, 2):
        ref, out = KH.clip_embed(mode, ids, seg_src, seg_pos0, own_off, own_len, 5, n + 2, tok, pos, eps)
        assert not ref
        out.assert_guards()
        if mode == 0:
            x = out["x"].reshape(n + 2, H)
            assert np.array_equal(x[:n].view(np.uint32), x32[:n].view(np.uint32))
        else:
            x = out["x"].view(np.uint16).reshape(n + 2, H)
            assert np.array_equal(x[:n], RR.f16_bits(x32[:n]).reshape(n, H))
        assert KH.untouched(out["x"].reshape(n + 2, -1)[n:]).all()
        stat = out["stat"].reshape(n + 2, 2)
        if mode < 2:
            assert KH.untouched(stat).all()
            continue
        assert KH.untouched(stat[n:]).all()
        stored = x[:n].view(np.float16).astype(np.float64)
        m, r, dm, rho = RR.stats_bound(stored, eps)
        em, er = np.abs(stat[:n, 0] - m) / dm, np.abs(stat[:n, 1] / r - 1) / rho
        _note(f"clip_embed stat mean H {H}", em.max()), _note(f"clip_embed stat rstd H {H}", er.max())
        print(f"[ratio] clip_embed stat H {H}: mean {em.max():.3f} rstd {er.max():.3f}")
        assert (em <= 1).all() and (er <= 1).all(), (float(em.max()), float(er.max()))
    tok6 = np.ones((V, 6), np.float32)
    ref, out = KH.clip_embed(0, ids, seg_src, seg_pos0, own_off, own_len, 5, n + 2, tok6, np.ones((stride, 6), np.float32))
    assert ref and _untouched(out)
    wide = np.ones((V, 1028), np.float32)
    ref, out = KH.clip_embed(2, ids, seg_src, seg_pos0, own_off, own_len, 5, n + 2, wide, np.ones((stride, 1028), np.float32), eps)
    assert ref and _untouched(out)   # the 2-byte path keeps 4 float4 per lane


# ---- vision helpers, normalisation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("p", [4, 2])
def test_im2col(prec, p):
    pix = np.random.default_rng(p).standard_normal((2, 3, 8, 8)).astype(np.float32)
    ref, out = KH.im2col(prec, pix, p)
    assert not ref
    out.assert_guards()
    exp = RR.im2col_ref(pix, p)
    assert RR.bits_equal(KH.Stored(prec, out["out"], exp.size).bits, RR.store_bits(prec, exp))
    ref, out = KH.im2col(prec, pix, 3)   # 3 does not tile 8
    assert ref and _untouched(out)


def test_vision_assemble():
    rng = np.random.default_rng(4)
    po = rng.standard_normal((2, 4, 64)).astype(np.float32)
    cls, pos = rng.standard_normal(64).astype(np.float32), rng.standard_normal((5, 64)).astype(np.float32)
    ref, out = KH.vision_assemble(po, cls, pos)
    assert not ref
    out.assert_guards()
    assert np.array_equal(out["x"].view(np.uint32), RR.vision_assemble_ref(po, cls, pos).reshape(-1).view(np.uint32))


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("D", [64, 512, 100])
def test_l2_normalize(M, D):
    x = (np.random.default_rng(D + M).standard_normal((M, D)) * 3).astype(np.float32)
    ref, out = KH.l2_normalize(x)
    assert not ref
    out.assert_guards()
    y64, tol = RR.l2_normalize_bound(x)
    _check(out["y"].reshape(M, D), y64, tol, "l2_normalize", f"M {M} D {D}")
