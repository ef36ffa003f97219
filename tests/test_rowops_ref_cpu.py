"""The host references and error bounds of tests/rowops_ref.py, checked without a GPU: a correct float32 LayerNorm in another
summation order stays inside the derived bound on every input the GPU test uses, each wrong variant leaves it, and the exact
storage / permutation helpers agree with torch."""
import numpy as np
import pytest
import torch

import rowops_ref as RR


@pytest.mark.parametrize("H", RR.LN_H)
@pytest.mark.parametrize("eps", RR.LN_EPS)
def test_float32_layernorm_in_another_order_stays_inside_the_bound(H, eps):
    x, g, b, idx = RR.ln_inputs(H)
    for ri in (None, idx):
        y64, tol = RR.layernorm_bound(x, g, b, eps, ri)
        y = RR.layernorm_f32(x, g, b, eps, ri)
        ok = RR.inside(y, y64, tol)
        assert ok.all(), (H, eps, np.nonzero(~ok)[0][:5], RR.worst_ratio(y, y64, tol))
        # the reference agrees with torch's float64 LayerNorm
        xs = torch.from_numpy(x if ri is None else x[ri]).double()
        t = torch.nn.functional.layer_norm(xs, (H,), torch.from_numpy(g).double(), torch.from_numpy(b).double(), eps).numpy()
        np.testing.assert_allclose(y64, t, rtol=1e-11, atol=1e-9)   # (the constant row: rstd = 1e6 times a 1e-16 residue)
    # the constant row's mean is exact, so y is beta bit for bit
    assert np.array_equal(RR.layernorm_f32(x, g, b, eps)[2], b)


@pytest.mark.parametrize("mutant", RR.MUTANTS)
def test_each_wrong_layernorm_leaves_the_bound(mutant):
    """every (H, eps) of the GPU test catches the variant on at least one of its rows, except where the variant is the identity
    (gamma / beta shifted by 4 columns at H = 4) or invisible in exact arithmetic too (eps = 1e-12 dropped from a row of spread >= 0.1
    changes y by 5e-11 relative: there only the constant row, 0 * inf, shows it)"""
    for H in RR.LN_H:
        for eps in RR.LN_EPS:
            if mutant == "gamma_shift" and H == 4:
                continue
            x, g, b, idx = RR.ln_inputs(H)
            y64, tol = RR.layernorm_bound(x, g, b, eps, idx)
            y = RR.layernorm_f32(x, g, b, eps, idx, mutant=mutant)
            broken = ~RR.inside(y, y64, tol)
            assert broken.any(), (mutant, H, eps, RR.worst_ratio(y, y64, tol))
            if mutant in ("h_minus_1", "gamma_shift"):   # these are wrong on every row that is not constant
                assert broken[idx != 2].all(), (mutant, H, eps)


def test_storage_roundings_are_the_ieee_ones():
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 4, 4096), [0.0, -0.0, 1.0, 65504.0, 2.0 ** -24, 2.0 ** -25]]).astype(np.float32)
    tb = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(RR.bf16_bits(v), tb)
    th = torch.from_numpy(v).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(RR.f16_bits(v), th)
    hi, lo = RR.split_bits(v)
    back = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)
    assert (np.abs(back - v) <= RR.storage_half_ulp(RR.F16X3, v.astype(np.float64))).all()
    for prec in (RR.BF16, RR.F16):
        bits = RR.store_bits(prec, v)
        val = (bits.astype(np.uint32) << 16).view(np.float32) if prec == RR.BF16 else bits.view(np.float16).astype(np.float32)
        assert (np.abs(val.astype(np.float64) - v) <= RR.storage_half_ulp(prec, v.astype(np.float64))).all()


def _ln_finalize_f32(part, M, eps):
    """ln_finalize_kernel in float32 numpy: sequential sums over the blocks, var = E[x^2] - mean^2 clamped at 0"""
    p = np.asarray(part, np.float32)[:, :M]
    s, q = p[0, :, 0].copy(), p[0, :, 1].copy()
    for b in range(1, p.shape[0]):
        s = s + p[b, :, 0]
        q = q + p[b, :, 1]
    n = np.float32(p.shape[0] * 32)
    mean = s / n
    var = np.maximum(q / n - mean * mean, np.float32(0))
    return mean, (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)


@pytest.mark.parametrize("M", [1, 255, 257])
def test_ln_finalize_in_float32_stays_inside_its_bound(M):
    _, ratio, part = RR.lnf_inputs(M, M + 3)
    m64, r64, dm, rho = RR.ln_finalize_bound(part, M, 1e-5)
    mean, rstd = _ln_finalize_f32(part, M, 1e-5)
    assert (np.abs(mean - m64) <= dm).all()
    rel = np.abs(rstd / r64 - 1)
    assert (rel <= rho).all(), float((rel / rho).max())
    # the bound grows with the cancellation: rho ~ u (1 + mean^2 / var)
    for q in RR.LNF_RATIOS:
        if (ratio == q).any():
            assert rho[ratio == q].max() < 40 * RR.U * (1 + q * q) * 1.5
    # and it is a bound on the partials' statistics, which are the rows' own
    x, _, _ = RR.lnf_inputs(M, M + 3)
    m, v, r = RR.row_stats64(x, 1e-5)
    np.testing.assert_allclose(m64, m, atol=1e-6)
    np.testing.assert_allclose(r64, r, rtol=1e-5)


def test_stats_bound_holds_for_float32_two_pass_statistics():
    for H in (64, 512, 768):
        x, _, _, _ = RR.ln_inputs(H)
        x = x.astype(np.float16).astype(np.float32)
        m, r, dm, rho = RR.stats_bound(x, 1e-5)
        mean = x.sum(-1, dtype=np.float32) / np.float32(H)
        d = x - mean[:, None]
        rstd = np.float32(1) / np.sqrt((d * d).sum(-1, dtype=np.float32) / np.float32(H) + np.float32(1e-5))
        assert (np.abs(mean - m) <= dm).all() and (np.abs(rstd / r - 1) <= rho).all()


@pytest.mark.parametrize("D", [64, 512, 100])
def test_l2_normalize_bound(D):
    x = np.random.default_rng(D).standard_normal((5, D)).astype(np.float32)
    y64, tol = RR.l2_normalize_bound(x)
    y = x / np.sqrt((x * x).sum(-1, dtype=np.float32, keepdims=True))
    assert (np.abs(y - y64) <= tol).all()
    assert not (np.abs(x / np.sqrt((x * x)[:, :-1].sum(-1, dtype=np.float32, keepdims=True)) - y64) <= tol).all()   # a dropped column shows


@pytest.mark.parametrize("p", [4, 2])
def test_im2col_is_the_patch_convolution(p):
    rng = np.random.default_rng(p)
    pix = rng.standard_normal((2, 3, 8, 8)).astype(np.float32)
    W = rng.standard_normal((5, 3, p, p)).astype(np.float32)
    conv = torch.nn.functional.conv2d(torch.from_numpy(pix).double(), torch.from_numpy(W).double(), stride=p)   # [B, 5, G, G]
    ref = conv.flatten(2).transpose(1, 2).reshape(-1, 5).numpy()
    got = RR.im2col_ref(pix, p).astype(np.float64) @ W.reshape(5, -1).astype(np.float64).T
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    assert sorted(RR.im2col_ref(pix, p).reshape(-1).tolist()) == sorted(pix.reshape(-1).tolist())   # a permutation


def test_embedding_references():
    rng = np.random.default_rng(9)
    word, pos, typ = (rng.standard_normal(s).astype(np.float32) for s in ((50, 64), (8, 64), (64,)))
    ids = np.array([[0, 49, 7], [3, 3, 1]])
    rows = RR.bert_embed_rows(ids, np.tile(np.arange(3), 2), word, pos, typ)
    assert rows.dtype == np.float32 and np.array_equal(rows[4], (word[3] + typ) + pos[1])
    x, wr = RR.clip_embed_rows(np.array([[1, 2, 3, 4], [5, 6, 7, 8]]), [1, 0], [1, 2], [0, 5], [2, 0], word, pos, 7)
    assert wr.tolist() == [True, True] + [False] * 5 and np.array_equal(x[1], word[7] + pos[2])
    po = rng.standard_normal((2, 4, 64)).astype(np.float32)
    va = RR.vision_assemble_ref(po, typ, pos[:5])
    assert np.array_equal(va[1, 0], typ + pos[0]) and np.array_equal(va[1, 3], po[1, 2] + pos[3])
