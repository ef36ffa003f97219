"""NumPy references of the caption-fluency kernels (csrc/fluency.hip), float64 throughout, and the inputs the kernel tests share.

logprob_ref: log softmax(x / t) at a target id and the id's rank by the engine's rule, rank = #{i : x_i > x_t} +
#{i < t : x_i == x_t} on the raw logits (ties in ascending id, the order of csrc/topk.hip).  logprob_f32: the same arithmetic
restated in plain fp32 with 256 strided partial sums, i.e. what a one-pass kernel can be asked to reach.  expand_ref: the
expansion of R captions into one masked sequence per word.
"""
import numpy as np

KERNEL_BAR = 5e-6   # |logp - ref64| of the kernel: half an ulp of y_t - m at magnitude up to 32 is 1.9e-6; the rest covers expf, logf and the tree sum
VOCABS = (1, 2, 63, 64, 65, 255, 1024, 1025, 4099, 30522)
TEMPS = (1.0, 0.1)


def logprob_ref(logits, target, temperature):
    """logits [N, V], target [N] -> (logp float64 [N], rank int64 [N])."""
    x = np.asarray(logits)
    t = np.asarray(target, dtype=np.int64)
    N, V = x.shape
    y = x.astype(np.float64) / float(temperature)
    m = y.max(axis=1)
    lse = m + np.log(np.exp(y - m[:, None]).sum(axis=1))
    rows = np.arange(N)
    logp = y[rows, t] - lse
    xt = x[rows, t][:, None]
    ids = np.arange(V)[None, :]
    rank = (x > xt).sum(axis=1) + ((x == xt) & (ids < t[:, None])).sum(axis=1)
    return logp, rank.astype(np.int64)


def logprob_f32(logits, target, temperature, lanes=256):
    """The reference's arithmetic in fp32: y = x / t rounded, the row maximum, `lanes` strided partial sums of exp(y - m), their
    pairwise sum, logp = (y_t - m) - log(s)."""
    x = np.asarray(logits, dtype=np.float32)
    N, V = x.shape
    t32 = np.float32(temperature)
    out = np.empty((N,), dtype=np.float32)
    for n in range(N):
        y = (x[n] / t32).astype(np.float32)
        m = y.max()
        e = np.exp((y - m).astype(np.float32)).astype(np.float32)
        part = np.zeros((lanes,), dtype=np.float32)
        for k in range(0, V, lanes):   # lane i adds elements i, i + lanes, ... in order
            seg = e[k:k + lanes]
            part[:seg.size] = (part[:seg.size] + seg).astype(np.float32)
        while part.size > 1:           # tree
            part = (part[0::2] + part[1::2]).astype(np.float32)
        out[n] = np.float32(np.float32(y[int(target[n])] - m) - np.float32(np.log(part[0])))
    return out


def kernel_case(N, V, temperature, seed):
    """The logits and targets of one (N, V, t) case of the kernel test: |x / t| <= 16, a run of equal values planted in every row,
    targets cycling through id 0, id V - 1, the row maximum, the row minimum and the inside of the run."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, V)) * 4.0).astype(np.float32)
    x = np.clip(x, -16.0, 16.0) * np.float32(temperature)
    x = np.clip(x, np.float32(-16.0 * temperature), np.float32(16.0 * temperature)).astype(np.float32)
    target = np.zeros((N,), dtype=np.int32)
    for n in range(N):
        run = min(V, 5)
        start = int(rng.integers(0, V - run + 1))
        x[n, start:start + run] = x[n, start]          # equal values at consecutive ids
        if V > 8:                                      # and the same value once more, far away
            x[n, (start + V // 2) % V] = x[n, start]
        kind = n % 5
        if kind == 0:
            target[n] = 0
        elif kind == 1:
            target[n] = V - 1
        elif kind == 2:
            target[n] = int(np.argmax(x[n]))
        elif kind == 3:
            target[n] = int(np.argmin(x[n]))
        else:
            target[n] = start + run // 2
    return x, target


def expand_ref(rows, seed_len, lens, mask_id):
    """rows int [R, T], lens [R] or None -> (ids [N, T], target [N], gen_rows [N]): sequence n = row r with word j masked, rows in
    order, j ascending; every other column as it stands."""
    rows = np.asarray(rows, dtype=np.int32)
    R, T = rows.shape
    lmax = T - seed_len - 1
    ln = [lmax] * R if lens is None else [int(v) for v in lens]
    ids, target, gen = [], [], []
    for r in range(R):
        for j in range(ln[r]):
            col = seed_len + j
            row = rows[r].copy()
            target.append(int(row[col]))
            row[col] = mask_id
            ids.append(row)
            gen.append(col)
    return np.stack(ids).astype(np.int32), np.array(target, dtype=np.int32), np.array(gen, dtype=np.int32)


# ---- end to end: the cases of tests/test_fluency_rows_gpu.py and their float64 oracle --------------------------------------
LOGIT_BAR = {"f32": 5e-5, "split": 2e-4}   # the project's own logit bars (tests/test_step_gpu.py test_bert_logits_row_vs_reference)
E2E_LENS = (1, 3, 6, 6, 4)
E2E_SEED_LEN = 4
E2E_T = E2E_SEED_LEN + max(E2E_LENS) + 1
# One seed per row, chosen so that the oracle's own near-ties leave out NO position at the split tower's bar (with 20 / 30 positions
# the 2 % allowance is less than one position; a random row has a near-tie at about one position in four, the tiny vocabulary's 640
# logits lie that close): for row r the first seed >= 100 r with that property at the row's length.  Asserted in test_fluency_cpu.py.
E2E_ROW_SEEDS = {"ragged": (1, 100, 201, 301, 403), "dense": (0, 114, 201, 301, 415)}


def e2e_lens(dense):
    return [max(E2E_LENS)] * len(E2E_LENS) if dense else list(E2E_LENS)


def e2e_row(special, regular_ids, L, seed, seed_len=E2E_SEED_LEN, T=E2E_T):
    """One row at stride T: [CLS], seed_len - 1 prompt words, L words, [SEP], then [PAD]; words drawn from `regular_ids`."""
    rng = np.random.default_rng(seed)
    row = np.full((T,), special["[PAD]"], dtype=np.int32)
    row[0] = special["[CLS]"]
    row[1:seed_len + L] = rng.choice(regular_ids, size=seed_len - 1 + L)
    row[seed_len + L] = special["[SEP]"]
    return row


def e2e_rows(special, regular_ids, dense):
    """The R = 5 rows of the end-to-end tests (ragged lengths E2E_LENS, or all of the longest length) -> (rows [R, T], lens)."""
    lens = e2e_lens(dense)
    seeds = E2E_ROW_SEEDS["dense" if dense else "ragged"]
    return np.stack([e2e_row(special, regular_ids, L, sd) for L, sd in zip(lens, seeds)]), lens


# The one full-size case (bert-base shapes, V = 30 522, synthetic weights of seed 11): R = 2 rows of L = 4 words behind a 3-word
# prompt.  Starting from e2e_row(seeds 700, 701) every word was replaced once, left to right, by the token the oracle ranks
# (0, 1, 2, 3) / (3, 0, 5, 1) at that moment; the oracle's ranks of the finished rows are (0, 22, 2, 3) / (1, 1, 18, 1) with every
# logit gap above twice the split tower's bar (among 30 522 random-init logits a random word is in a near-tie almost surely).
FULL_SEED_LEN, FULL_L = 4, 4
FULL_ROWS = ((101, 8246, 8876, 21208, 14332, 18765, 14332, 23449, 102), (101, 3659, 28274, 21907, 27968, 14332, 21797, 14332, 102))


def oracle_fluency(bert_w, cfg, rows, seed_len, lens, mask_id, temperature, logit_bar):
    """The float64 oracle of czc_fluency_rows: oracle.models.bert_mlm_logits on each row's own T_r tokens with word j masked, then
    logprob_ref.  Returns (logp [R, Lmax] padded with 0, rank [R, Lmax] padded with -1, sure [R, Lmax] bool: the oracle's logit
    gap from the target to both of its neighbours in the sorted candidate list exceeds twice `logit_bar`, logits: dict
    (r, j) -> float64 [V])."""
    import torch
    from oracle import models as M
    w = {k: (v.double() if v.is_floating_point() else v) for k, v in M.to_torch(bert_w).items()}
    rows = np.asarray(rows)
    R, T = rows.shape
    lmax = T - seed_len - 1
    ln = [lmax] * R if lens is None else [int(v) for v in lens]
    logp, rank = np.zeros((R, lmax)), np.full((R, lmax), -1, dtype=np.int64)
    sure = np.zeros((R, lmax), dtype=bool)
    logits = {}
    for r in range(R):
        Tr = seed_len + ln[r] + 1
        seqs = np.repeat(rows[r:r + 1, :Tr].astype(np.int64), ln[r], axis=0)
        tgt = np.empty((ln[r],), dtype=np.int64)
        for j in range(ln[r]):
            tgt[j] = seqs[j, seed_len + j]
            seqs[j, seed_len + j] = mask_id
        with torch.no_grad():
            x = M.bert_mlm_logits(w, cfg, torch.from_numpy(seqs), rows=range(seed_len, seed_len + ln[r]))
            x = x[torch.arange(ln[r]), torch.arange(ln[r])].numpy()   # sequence j: its masked row
        lp, rk = logprob_ref(x, tgt, temperature)
        logp[r, :ln[r]], rank[r, :ln[r]] = lp, rk
        for j in range(ln[r]):
            order = np.lexsort((np.arange(x.shape[1]), -x[j]))   # by logit descending, id ascending
            at = int(rk[j])
            assert order[at] == tgt[j]
            gaps = [abs(x[j, order[k]] - x[j, tgt[j]]) for k in (at - 1, at + 1) if 0 <= k < x.shape[1]]
            sure[r, j] = min(gaps) > 2 * logit_bar if gaps else True
            logits[(r, j)] = x[j]
    return logp, rank, sure, logits
