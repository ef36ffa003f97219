"""-m gpu: czc_score_rows (include/conzic_hip.h) -- the CLIP cosine of BERT-id rows with their images, all on the device.  Tiny
synthetic towers, six rows over two images.  The yardsticks: the host bridge (oracle.text.bridge) -> Engine.encode_text -> an
fp64 cosine (the same tower on the same rows, so only the fp32 dot differs: 2e-6, the project's fp32-cosine bar) and, on F32,
oracle.models.clip_text_embeds (something that is not this engine: 2e-5, the bound of the trajectory goldens)."""
import numpy as np
import pytest
import torch

from conzic_amd import harness, lengths, native, synth
from oracle import models as M, text as T

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT, REFINE = native.PREC_F32, native.PREC_BF16, native.PREC_SPLIT, native.PREC_REFINE
PROMPT = "Image of a"
SEED_LEN = 4
LENS = [1, 3, 6, 6, 4, 2]
IOR = np.array([0, 1, 0, 0, 1, 1], dtype=np.int32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _setup(prec):
    su = harness.build_synthetic(True, prec)
    emb = np.random.default_rng(3).standard_normal((2, su.clip_cfg.proj)).astype(np.float32)
    su.engine.set_image_embeds(emb)
    return su, emb


def _rows(su):
    """Lengths LENS: rows 0, 1, 2, 3 fully worded (2 and 3 identical), row 4 with two [MASK]s left, row 5 all [MASK] (it
    decodes to the prompt only)."""
    rows = lengths.length_rows(su.bert_tok, PROMPT, LENS)
    regular = np.nonzero(su.token_mask[0] > 0)[0]
    rng = np.random.default_rng(17)
    for r in (0, 1, 2, 4):
        rows[r, SEED_LEN:SEED_LEN + LENS[r]] = rng.choice(regular, size=LENS[r])
    rows[3] = rows[2]
    mask_id = harness.special_ids(su.bert_tok)["[MASK]"]
    rows[4, [SEED_LEN + 1, SEED_LEN + 3]] = mask_id
    assert (rows[5, SEED_LEN:SEED_LEN + LENS[5]] == mask_id).all()
    return np.ascontiguousarray(rows)


def _clip_ids(su, rows, lens):
    bpe = T.ClipBpe(su.sv.clip_vocab, su.sv.clip_merges)
    out = [T.bridge([int(t) for t in rows[r, :SEED_LEN + n + 1]], su.sv.bert_tokens, bpe) for r, n in enumerate(lens)]
    ids = np.full((len(out), max(len(o) for o in out)), su.clip_cfg.eos_id, dtype=np.int32)
    for r, o in enumerate(out):
        ids[r, :len(o)] = o
    return ids, np.array([len(o) for o in out], dtype=np.int32)


def _cos64(text, img):
    t, i = np.asarray(text, np.float64), np.asarray(img, np.float64)
    return (t * i).sum(1) / np.linalg.norm(t, axis=1) / np.linalg.norm(i, axis=1)


@pytest.mark.parametrize("prec", [F32, BF16, SPLIT, REFINE])
def test_against_the_host_bridge_and_encode_text(prec):
    su, emb = _setup(prec)
    eng = su.engine
    try:
        rows = _rows(su)
        got = eng.score_rows(rows, SEED_LEN, LENS, IOR)
        cids, clen = _clip_ids(su, rows, LENS)
        assert clen[5] == len(T.ClipBpe(su.sv.clip_vocab, su.sv.clip_merges).encode(PROMPT))   # all [MASK]: the prompt only
        want = _cos64(eng.encode_text(cids, clen), emb[IOR])
        err = np.abs(got.astype(np.float64) - want)
        print(f"[score_rows] prec {prec}: worst |d cos| against bridge -> encode_text -> fp64 cosine {err.max():.3e}")
        assert got.dtype == np.float32 and got.shape == (6,)
        assert err.max() <= 2e-6
        np.testing.assert_array_equal(_bits(got[2]), _bits(got[3]))   # identical rows, one image
    finally:
        eng.close()


def test_f32_against_the_cpu_oracle():
    su, emb = _setup(F32)
    eng = su.engine
    try:
        rows = _rows(su)
        got = eng.score_rows(rows, SEED_LEN, LENS, IOR)
        cids, clen = _clip_ids(su, rows, LENS)
        w = M.to_torch(synth.make_clip_weights(su.clip_cfg, 12))
        ref = M.clip_text_embeds(w, su.clip_cfg, torch.from_numpy(cids.astype(np.int64)), torch.from_numpy(clen.astype(np.int64)))
        err = np.abs(got.astype(np.float64) - _cos64(ref.double().numpy(), emb[IOR]))
        print(f"[score_rows] F32: worst |d cos| against oracle.models.clip_text_embeds {err.max():.3e}")
        assert err.max() <= 2e-5
    finally:
        eng.close()


def test_one_row_one_image_for_all_rows_and_independence():
    """R = 1 (identity image map); image_of_row naming one image for all rows; a row scored alone, in the batch, under
    another index and from device memory returns the same bits (F32)."""
    su, emb = _setup(F32)
    eng = su.engine
    try:
        rows = _rows(su)
        full = eng.score_rows(rows, SEED_LEN, LENS, IOR)
        one_img = eng.score_rows(rows, SEED_LEN, LENS, np.ones(6, dtype=np.int32))
        cids, clen = _clip_ids(su, rows, LENS)
        want = _cos64(eng.encode_text(cids, clen), emb[np.ones(6, dtype=np.int64)])
        assert np.abs(one_img.astype(np.float64) - want).max() <= 2e-6
        np.testing.assert_array_equal(_bits(one_img[IOR == 1]), _bits(full[IOR == 1]))
        for r in range(6):
            alone = eng.score_rows(rows[r:r + 1], SEED_LEN, [LENS[r]], [int(IOR[r])])
            np.testing.assert_array_equal(_bits(alone), _bits(full[r:r + 1]))
        perm = np.array([4, 0, 5, 2, 1, 3])
        np.testing.assert_array_equal(_bits(eng.score_rows(rows[perm], SEED_LEN, [LENS[i] for i in perm], IOR[perm])), _bits(full[perm]))
        dev = torch.from_numpy(rows).cuda()
        np.testing.assert_array_equal(_bits(eng.score_rows(dev, SEED_LEN, LENS, IOR)), _bits(full))
        # lens = None: every row has T tokens (the uniform rows 2 and 3); identity image map with R == resident batch
        pair = eng.score_rows(rows[[2, 3]], SEED_LEN)
        np.testing.assert_array_equal(_bits(pair[0]), _bits(full[2]))
        eng.set_image_embeds(emb[:1])
        np.testing.assert_array_equal(_bits(eng.score_rows(rows[2:3], SEED_LEN)), _bits(full[2:3]))   # R = 1, no maps at all
    finally:
        eng.close()


def test_argument_errors_leave_the_engine_usable():
    su, emb = _setup(F32)
    eng = su.engine
    try:
        rows = _rows(su)
        good = eng.score_rows(rows, SEED_LEN, LENS, IOR)
        V = len(su.sv.bert_tokens)
        T_ = rows.shape[1]

        def refused(code, r, lens, ior, seed_len=SEED_LEN):
            with pytest.raises(native.NativeError) as ei:
                eng.score_rows(r, seed_len, lens, ior)
            assert ei.value.code == code, ei.value
            np.testing.assert_array_equal(_bits(eng.score_rows(rows, SEED_LEN, LENS, IOR)), _bits(good))

        for bad_id in (V, -1):
            bad = rows.copy()
            bad[1, SEED_LEN] = bad_id
            refused(native.ERR_ARG, bad, LENS, IOR)
        refused(native.ERR_ARG, rows, [0] + LENS[1:], IOR)
        refused(native.ERR_ARG, rows, LENS[:5] + [T_ - SEED_LEN], IOR)
        refused(native.ERR_ARG, rows, LENS, [0, 1, 0, 0, 1, 2])
        refused(native.ERR_ARG, rows, LENS, [0, 1, 0, 0, 1, -1])
        refused(native.ERR_ARG, rows, LENS, None)                           # identity map needs R == resident batch
        many = np.repeat(rows[:1], 16384 + 1, axis=0)
        refused(native.ERR_ARG, many, None, np.zeros(16384 + 1, dtype=np.int32))
        wide = np.zeros((1, native.MAX_BERT_LEN + 1), dtype=np.int32)
        refused(native.ERR_ARG, wide, None, [0])
    finally:
        eng.close()
    su = harness.build_synthetic(True, F32)     # no image embeds yet: CZC_ERR_STATE, then a successful call
    try:
        with pytest.raises(native.NativeError) as ei:
            su.engine.score_rows(rows, SEED_LEN, LENS, IOR)
        assert ei.value.code == native.ERR_STATE
        su.engine.set_image_embeds(emb)
        np.testing.assert_array_equal(_bits(su.engine.score_rows(rows, SEED_LEN, LENS, IOR)), _bits(good))
    finally:
        su.engine.close()
