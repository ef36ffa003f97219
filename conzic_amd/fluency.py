"""Caption fluency on the host side: what to make of Engine.fluency_rows' arrays.

BERT's pseudo-log-likelihood PLL(w) = sum_j log p(w_j | w with word j masked) is the standard sentence score of a masked LM and
the conditional every Gibbs step of the engine evaluates.  Engine.fluency_rows returns log p and the rank of every word;
summarize() reduces them per caption, pick() chooses among the samples of an image by cosine and fluency together.  NumPy only.
"""
from typing import Optional, Sequence

import numpy as np


def summarize(logp, rank, lens: Optional[Sequence[int]] = None):
    """Per caption, from logp / rank [R, Lmax] (columns behind a caption's lens[r] words are ignored; None: all Lmax count):
    a list of dicts with `pll` (sum of log p), `mean_logp`, `ppl` = exp(-mean_logp) (pseudo-perplexity), `worst_pos` and
    `worst_rank` (the word BERT ranks lowest; the first such word on ties), `len`.  Sums are float64, in column order."""
    lp = np.asarray(logp, dtype=np.float64)
    rk = np.asarray(rank, dtype=np.int64)
    if lp.ndim != 2 or rk.shape != lp.shape or lp.shape[1] < 1:
        raise ValueError(f"summarize: logp and rank must be [R, Lmax] alike, got {lp.shape} and {rk.shape}")
    R, lmax = lp.shape
    ln = np.full((R,), lmax, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64).reshape(-1)
    if ln.size != R or (R and (ln.min() < 1 or ln.max() > lmax)):
        raise ValueError(f"summarize: lens must hold {R} lengths in [1, {lmax}]")
    out = []
    for r in range(R):
        n = int(ln[r])
        pll = 0.0
        for j in range(n):
            pll += float(lp[r, j])
        mean = pll / n
        worst = int(np.argmax(rk[r, :n]))   # first index on ties
        out.append(dict(pll=pll, mean_logp=mean, ppl=float(np.exp(-mean)), worst_pos=worst, worst_rank=int(rk[r, worst]), len=n))
    return out


def pick(cos, mean_logp, lam: float) -> int:
    """Index of the largest cos[i] + lam * mean_logp[i]; the first index on ties."""
    c = np.asarray(cos, dtype=np.float64).reshape(-1)
    m = np.asarray(mean_logp, dtype=np.float64).reshape(-1)
    if c.size < 1 or m.size != c.size:
        raise ValueError(f"pick: cos and mean_logp must hold the same number (>= 1) of samples, got {c.size} and {m.size}")
    if not np.isfinite(lam):
        raise ValueError("pick: lam must be finite")
    return int(np.argmax(c + float(lam) * m))
