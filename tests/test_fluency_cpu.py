"""Caption fluency (czc_fluency_rows): the references, conzic_amd/fluency.py, the binding and the command-line refusals.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import fluency_ref as FR
from conzic_amd import fluency, harness, native, synth
from conzic_amd.demo_cli import get_args


def test_fp32_restatement_stays_within_the_kernel_bar():
    """The bar of tests/test_logprob_kernel_gpu.py is one plain fp32 arithmetic can meet: the reference restated in fp32 with 256
    strided partial sums, on that test's own inputs, against the float64 reference."""
    worst = 0.0
    for V in (1, 2, 63, 65, 1025, 4099, 30522):
        for t in FR.TEMPS:
            x, target = FR.kernel_case(3, V, t, seed=V)
            assert np.abs(x / np.float32(t)).max() <= 16.0 * (1 + 1e-6)
            ref, _ = FR.logprob_ref(x, target, t)
            worst = max(worst, float(np.abs(FR.logprob_f32(x, target, t).astype(np.float64) - ref).max()))
    print(f"fp32 restatement: worst |logp - ref64| = {worst:.2e}")
    assert worst < FR.KERNEL_BAR


def test_rank_on_planted_ties_and_duplicates():
    x = np.array([[1.0, 3.0, 3.0, 0.5, 3.0, -2.0, 1.0]], dtype=np.float32)
    for target, want in ((1, 0), (2, 1), (4, 2), (0, 3), (6, 4), (3, 5), (5, 6)):
        _, rank = FR.logprob_ref(x, [target], 1.0)
        assert rank[0] == want, (target, rank[0], want)
    # rank r = the r-th entry of the list sorted by (logit descending, id ascending); temperature does not move it
    rng = np.random.default_rng(0)
    y = np.round(rng.standard_normal((4, 50)) * 2).astype(np.float32)   # many duplicates
    for n in range(4):
        order = np.lexsort((np.arange(50), -y[n]))
        for t in (0.1, 1.0):
            _, rank = FR.logprob_ref(np.repeat(y[n:n + 1], 50, axis=0), np.arange(50), t)
            assert (order[rank] == np.arange(50)).all()
    lp, _ = FR.logprob_ref(np.zeros((1, 8), np.float32), [3], 0.5)
    assert abs(lp[0] + np.log(8.0)) < 1e-15
    one, rank = FR.logprob_ref(np.array([[2.5]], np.float32), [0], 0.1)   # V = 1
    assert one[0] == 0.0 and rank[0] == 0


def test_expand_ref_masks_one_word_per_sequence():
    rows = np.arange(2 * 7, dtype=np.int32).reshape(2, 7) + 10
    ids, target, gen = FR.expand_ref(rows, 2, [1, 3], 99)
    assert ids.shape == (4, 7) and target.tolist() == [12, 19, 20, 21] and gen.tolist() == [2, 2, 3, 4]
    assert (ids[0] == [10, 11, 99, 13, 14, 15, 16]).all() and (ids[3] == [17, 18, 19, 20, 99, 22, 23]).all()
    assert FR.expand_ref(rows, 2, None, 99)[0].shape == (8, 7)


def test_summarize_on_hand_made_arrays():
    logp = np.array([[-1.0, -3.0, 0.0], [-0.5, -0.5, -2.0]], dtype=np.float32)
    rank = np.array([[0, 7, -1], [4, 4, 1]], dtype=np.int32)
    a, b = fluency.summarize(logp, rank, [2, 3])
    assert a["pll"] == -4.0 and a["mean_logp"] == -2.0 and a["ppl"] == pytest.approx(np.exp(2.0)) and a["len"] == 2
    assert (a["worst_pos"], a["worst_rank"]) == (1, 7)
    assert b["pll"] == -3.0 and b["mean_logp"] == -1.0 and (b["worst_pos"], b["worst_rank"]) == (0, 4)   # first index on ties
    full = fluency.summarize(logp, rank)   # lens None: every column counts
    assert full[0]["len"] == 3 and full[0]["pll"] == -4.0
    for bad in ([2], [0, 3], [2, 4]):
        with pytest.raises(ValueError):
            fluency.summarize(logp, rank, bad)
    with pytest.raises(ValueError):
        fluency.summarize(logp, rank[:, :2])


def test_pick_weighs_cosine_and_fluency():
    cos, mean = [0.30, 0.32, 0.31], [-2.0, -6.0, -2.5]
    assert fluency.pick(cos, mean, 0.0) == 1          # the largest cosine
    assert fluency.pick(cos, mean, 0.01) == 2         # 0.28 / 0.26 / 0.285
    assert fluency.pick(cos, mean, 0.05) == 0         # 0.20 / 0.02 / 0.185
    assert fluency.pick(cos, mean, -1.0) == 1
    assert fluency.pick([0.2, 0.2, 0.2], [-1.0, -1.0, -1.0], 0.5) == 0   # first index on ties
    assert fluency.pick([0.1, 0.3, 0.3], [0.0, 0.0, 0.0], 2.0) == 1
    assert fluency.pick([0.4], [-9.0], 3.0) == 0      # a single sample
    for bad in (([], [], 0.0), ([0.1], [0.1, 0.2], 0.0), ([0.1], [0.1], float("nan"))):
        with pytest.raises(ValueError):
            fluency.pick(*bad)


def test_library_binding_of_fluency_rows():
    lib = native.load()
    assert lib.czc_version() >= 107
    fn = lib.czc_fluency_rows
    res, args = native.SIGNATURES["czc_fluency_rows"]
    assert fn.restype is res and list(fn.argtypes) == args
    assert args == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    hdr = open(native.HEADER_PATH).read()
    decl = re.search(r"int czc_fluency_rows\(([^;]*)\);", hdr).group(1)
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert len(params) == len(args)
    kinds = [C.c_float if p.startswith("float ") and "*" not in p else C.c_int if p.startswith("int ") else C.c_void_p for p in params]
    assert kinds == args, params
    out = np.zeros(4, np.float32)
    assert fn(None, None, 1, 4, 1, None, 1.0, out.ctypes.data, None, None) == native.ERR_ARG   # no engine: refused, no GPU touched
    test = native.load_test()
    assert hasattr(test, "czc_test_logprob") and hasattr(test, "czc_test_expand_mask")
    assert "czc_test_logprob" in native.TEST_SIGNATURES and "czc_test_expand_mask" in native.TEST_SIGNATURES


def test_cli_defaults_and_the_implied_flag():
    a = get_args(["--synthetic"])
    assert a.fluency is False and a.pick_lambda is None
    assert get_args(["--synthetic", "--fluency"]).fluency is True
    a = get_args(["--synthetic", "--pick_lambda", "0.05", "--samples_num", "3"])
    assert a.fluency is True and a.pick_lambda == 0.05
    a = get_args(["--synthetic", "--fluency", "--batch_samples", "--sample_tau", "0.5", "--distinct", "1.0", "--run_type", "controllable"])
    assert a.fluency and a.batch_samples and a.sample_tau == 0.5 and a.distinct == 1.0
    assert get_args(["--synthetic", "--pick_lambda", "0"]).pick_lambda == 0.0   # samples_num defaults to 2


@pytest.mark.parametrize("argv", [
    ["--fluency", "--sentence_lens", "4,6"],
    ["--fluency", "--signals", "caption,positive"],
    ["--fluency", "--block_width", "2", "--order", "sequential"],
    ["--fluency", "--run_type", "infill", "--caption", "a _ dog", "--order", "sequential"],
    ["--fluency", "--run_type", "retrieve", "--index_captions", "x.txt"],
    ["--pick_lambda", "0.1", "--sentence_lens", "4,6"],
    ["--pick_lambda", "0.1", "--samples_num", "1"],
    ["--pick_lambda", "nan"],
    ["--pick_lambda", "inf"],
])
def test_cli_refusals(argv, capsys):
    with pytest.raises(SystemExit) as ei:
        get_args(["--synthetic"] + argv)
    assert ei.value.code == 2
    err = capsys.readouterr().err
    assert "--fluency" in err or "--pick_lambda" in err


@pytest.mark.parametrize("temperature", [1.0, 0.5])
@pytest.mark.parametrize("dense", [False, True])
def test_oracle_leaves_out_few_positions_on_the_gpu_tests_seeds(dense, temperature):
    """tests/test_fluency_rows_gpu.py compares ranks only where the oracle's own logit gaps exceed twice the logit bar and may leave
    out at most 2 % of the positions: on its rows and seeds the oracle alone leaves out fewer (here: none)."""
    sv = harness.cached_vocab(True)
    cfg = synth.bert_tiny(len(sv.bert_tokens))
    bt, _ = harness.tokenizers_from_vocab(sv)
    sp = harness.special_ids(bt)
    regular = np.nonzero(synth.make_token_mask(sv)[0] > 0)[0]
    rows, lens = FR.e2e_rows(sp, regular, dense)
    logp, rank, sure, _ = FR.oracle_fluency(synth.make_bert_weights(cfg, 11), cfg, rows, FR.E2E_SEED_LEN, lens, sp["[MASK]"], temperature,
                                            FR.LOGIT_BAR["split"])
    n = sum(lens)
    assert sure.sum() + 0.02 * n > n and sure.sum() == n
    for r, L in enumerate(lens):
        assert (rank[r, :L] >= 0).all() and (rank[r, L:] == -1).all() and (logp[r, L:] == 0).all() and (logp[r, :L] < 0).all()
