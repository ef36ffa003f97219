"""Harness-side assembly: build an engine from (synthetic or caller-provided) state dicts and
tokenizers.  This is the counterpart of what demo.py:125-143 does before it calls the boundary
(load models, build token_mask); shared by tests, bench.py, __graft_entry__.smoke() and the
drop-in modules at the repo root."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import native, synth
from .bridge import BridgeArrays, tables_from_tokenizers
from .engine import Engine
from .text import ClipBpeTokenizer, WordPieceTokenizer, tokenizers_from_vocab


@dataclass
class SynthSetup:
    engine: Engine
    sv: synth.SynthVocab
    bert_cfg: synth.BertCfg
    clip_cfg: synth.ClipCfg
    bert_tok: WordPieceTokenizer
    clip_tok: ClipBpeTokenizer
    tables: BridgeArrays
    token_mask: np.ndarray  # [1,V]


def special_ids(bert_tok) -> dict:
    sp = {k: int(bert_tok.vocab[k]) for k in ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", ".")}
    return sp


_vocab_cache = {}


def cached_vocab(tiny: bool) -> synth.SynthVocab:
    if tiny not in _vocab_cache:
        _vocab_cache[tiny] = synth.make_vocab_tiny() if tiny else synth.make_vocab()
    return _vocab_cache[tiny]


def build_synthetic(tiny: bool, precision: int = native.PREC_BF16, bseed: int = 11, cseed: int = 12,
                    logit_scale: float = 2.6592, regular_only: bool = False, lexicon: bool = False,
                    device: int = 0, bert_w=None, clip_w=None, bert_cfg=None, clip_cfg=None) -> SynthSetup:
    sv = cached_vocab(tiny)
    if bert_cfg is None:
        bert_cfg = synth.bert_tiny(len(sv.bert_tokens)) if tiny else synth.bert_base()
    if clip_cfg is None:
        clip_cfg = synth.clip_tiny(len(sv.clip_vocab)) if tiny else synth.clip_b32()
    clip_cfg.logit_scale = logit_scale
    bt, ct = tokenizers_from_vocab(sv)
    eng = Engine(bert_cfg, clip_cfg, special_ids(bt), precision, device)
    eng.load_state(bert_w if bert_w is not None else synth.make_bert_weights(bert_cfg, bseed))
    eng.load_state(clip_w if clip_w is not None else synth.make_clip_weights(clip_cfg, cseed))
    eng.finalize()
    tables = tables_from_tokenizers(bt, ct)
    eng.set_bridge(tables)
    mask = synth.make_token_mask(sv, regular_only=regular_only)
    eng.set_token_mask(mask)
    if lexicon:
        eng.set_lexicon(synth.make_lexicon(len(sv.bert_tokens)))
    return SynthSetup(eng, sv, bert_cfg, clip_cfg, bt, ct, tables, mask)


OUTLIER_CHANNELS = (7, 93, 200, 301, 402, 499)


def outlier_clip_weights(clip_cfg, cseed: int = 12, gain: float = 1.0):
    """CLIP weights of seed `cseed` with six channels of every TEXT-tower LayerNorm gain multiplied by `gain`: the activation
    outlier channels trained checkpoints have (a few LayerNorm gains tens of times the rest), which a single-pass fp16 tower
    rounds more coarsely (tests/test_step_gpu.py, tools/refine_validate.py; gain 1 = the plain draw)."""
    cw = synth.make_clip_weights(clip_cfg, cseed)
    if gain != 1.0:
        ch = np.array(OUTLIER_CHANNELS)
        for n in range(clip_cfg.layers):
            for ln in ("layer_norm1", "layer_norm2"):
                k = f"text_model.encoder.layers.{n}.{ln}.weight"
                g = np.array(cw[k], dtype=np.float32, copy=True)
                g[ch] *= gain
                cw[k] = g
    return cw


def order_positions(order: str, L: int, iters: int, order_list=None, random_positions=None):
    """(positions, n_mask, snapshot_every) for czc_generate from the reference's visiting orders
    (gen_utils.py:64-65 sequential, :110-115 shuffle, :160-166 span, :209-210 random)."""
    if order == "sequential":
        lst = list(range(L))
        return lst * iters, [1] * (L * iters), L
    if order == "shuffle":
        lst = list(order_list)
        assert sorted(lst) == list(range(L))
        return lst * iters, [1] * (L * iters), L
    if order == "span":
        pos, nm = [], []
        for s in range(0, L, 2):
            e = min(s + 2, L)
            pos.append(s)
            nm.append(e - s)
            if e - s == 2:
                pos.append(s + 1)
                nm.append(0)
        return pos * iters, nm * iters, L
    if order == "random":
        pos = [int(p) for p in random_positions]
        assert len(pos) == L * iters
        return pos, [1] * len(pos), L
    raise ValueError(order)


def sample_schedules(order: str, L: int, max_iters: int, S: int):
    """Visiting orders of S samples of one *_generation call each, drawn in the order and from the process-global RNG streams
    the serial sample loop would (demo.py:83 / run.py around the call): one `random.shuffle` per sample for `shuffle`
    (gen_utils.py:110-111), `max_iters` `np.random.randint` per sample for `random` (gen_utils.py:210; `max_iters` as the
    *_generation function receives it: steps for `random`, sweeps otherwise), nothing for `sequential` / `span`.  Afterwards
    both streams are where S serial calls would have left them.  Returns (positions int32 [n_steps, S] for
    czc_generate_rows, n_mask [n_steps], snapshot_every, order_lists: the S shuffled lists, or None)."""
    import random
    cols, order_lists, n_mask, every = [], ([] if order == "shuffle" else None), None, None
    for _ in range(S):
        if order == "shuffle":
            order_list = list(range(L))
            random.shuffle(order_list)
            order_lists.append(order_list)
            pos, n_mask, every = order_positions(order, L, max_iters, order_list=order_list)
        elif order == "random":
            pos = [int(np.random.randint(0, L)) for _ in range(max_iters)]
            n_mask, every = [1] * len(pos), 1
        else:
            pos, n_mask, every = order_positions(order, L, max_iters)
        cols.append(pos)
    positions = np.ascontiguousarray(np.array(cols, dtype=np.int32).reshape(S, -1).T)
    return positions, list(n_mask), every, order_lists


def first_divergence(engine, emb_row, init_row, ref_snaps, got_snaps, L, seed_len, K, hp, positions_per_sweep=None):
    """Where and how closely one image left a reference trajectory.  `ref_snaps` / `got_snaps`: int32 [S, T] per-sweep snapshots
    of that image from the reference engine (`engine`, e.g. the all-split one) and from the engine under test, sequential
    (or `positions_per_sweep`) order.  Replays `engine` ALONE on the image from the last common snapshot up to the first
    position whose token differs and returns what the reference engine saw there: its top-2 margin and the gap between its
    winner and the token the other engine wrote -- a gap inside the fused-score bar is a near-tie, i.e. inside the stated
    tolerance ("identical argmax ids" can only hold where the margin exceeds the error bound).  None if the snapshots agree."""
    ref_snaps, got_snaps = np.asarray(ref_snaps), np.asarray(got_snaps)
    diff = np.nonzero((ref_snaps != got_snaps).any(axis=1))[0]
    if diff.size == 0:
        return None
    s = int(diff[0])
    order = list(positions_per_sweep) if positions_per_sweep is not None else list(range(L))
    p_idx = next(i for i, p in enumerate(order) if ref_snaps[s][seed_len + p] != got_snaps[s][seed_len + p])
    cur = np.ascontiguousarray((ref_snaps[s - 1] if s > 0 else np.asarray(init_row))[None, :], dtype=np.int32).copy()
    engine.set_image_embeds(np.ascontiguousarray(emb_row[None, :], dtype=np.float32))
    r = None
    for i in range(p_idx + 1):
        p = order[i]
        r = engine.step(cur, seed_len + p, K, hp, dot_allowed=(p == L - 1), want=("cand_ids", "final_score", "best"))
        if i < p_idx and cur[0, seed_len + p] != ref_snaps[s][seed_len + p]:
            return dict(sweep=s, position=int(p), replay_mismatch=True)  # the single-image replay left the batch's trajectory itself
    fin, cand = r["final_score"][0], r["cand_ids"][0]
    srt = np.sort(fin)[::-1]
    other = int(got_snaps[s][seed_len + order[p_idx]])
    where = np.nonzero(cand == other)[0]
    gap = float(srt[0] - fin[where].max()) if where.size else None
    return dict(sweep=s, position=int(order[p_idx]), reference_top2_margin=float(srt[0] - srt[1]),
                gap_to_other_engines_choice=gap, other_choice_rank=(int((fin > fin[where].max()).sum()) if where.size else None))


# ---- option "memo" (czc_generate's exact step memo) ------------------------------------------------------------------------
MEMO_SUB = 2  # steps per (n_mask >= 1 step + its n_mask = 0 followers) group the engine's entries hold (engine.hip)


def memo_groups(n_mask, n_steps: int):
    """[(first step, number of steps)] of the step groups of czc_generate: one n_mask >= 1 step and the n_mask = 0 steps that
    re-use its forward (span order, gen_utils.py:160-179)."""
    nm = [1] * n_steps if n_mask is None else [int(x) for x in n_mask]
    out, s = [], 0
    while s < n_steps:
        g = 1
        while s + g < n_steps and nm[s + g] <= 0:
            g += 1
        out.append((s, g))
        s += g
    return out


def memo_refine_no_hit(n_steps: int, snapshot_every: int, want_cos: bool = True) -> np.ndarray:
    """Steps of a CZC_PREC_REFINE czc_generate call that never hit (include/conzic_hip.h, option "memo"): its audit steps and
    the steps whose winner cosine the call returns."""
    never = np.zeros(n_steps, bool)
    audited = False
    for s in range(n_steps):
        snap = (s + 1) % snapshot_every == 0
        audit = (snap and (s // snapshot_every) % 4 == 0) or (s + 1 == n_steps and not audited)
        audited = audited or audit
        never[s] = audit or (snap and want_cos)
    return never


def memo_expected_hits(snapshots, positions, n_mask, seed_len: int, mask_id: int, never=None) -> np.ndarray:
    """The memo rule stated on the host.  `snapshots` int32 [n_steps, B, T]: a memo-OFF trajectory recorded with
    snapshot_every = 1 (row of every image after every step).  Returns bool [n_steps, B]: whether image b hits at step s
    (the engine's czc_memo_stats counts their sum).

    Step s at position p with n_mask = m >= 1 sees R_s(b) = the row before the step with columns seed_len+p .. seed_len+p+m-1
    set to [MASK].  Its key is the (position, n_mask) list of its group (the step and the n_mask = 0 steps that follow it);
    image b hits when an earlier group of the call had the same key and left R(b) equal to R_s(b), bit for bit.  Every step
    of a group hits with its first step; a group with more than MEMO_SUB steps, a group that does not start with n_mask >= 1
    and a group with a step in `never` (bool [n_steps]) do not hit.  Every visit replaces the entry."""
    snaps = np.asarray(snapshots)
    n_steps, B, T = snaps.shape
    assert len(positions) == n_steps
    nm = [1] * n_steps if n_mask is None else [int(x) for x in n_mask]
    never = np.zeros(n_steps, bool) if never is None else np.asarray(never, bool)
    hits = np.zeros((n_steps, B), bool)
    entries = {}
    for s, g in memo_groups(nm, n_steps):
        if nm[s] < 1 or g > MEMO_SUB:
            continue
        key = tuple((int(positions[s + j]), nm[s + j]) for j in range(g))
        # a step writes inside the columns it masked only, so the row it left, masked again, is the row it saw
        rows = snaps[s].copy()
        c0 = seed_len + int(positions[s])
        rows[:, c0:min(c0 + nm[s], T)] = mask_id
        prev = entries.get(key)
        if prev is not None and not never[s:s + g].any():
            hits[s:s + g] = (prev == rows).all(axis=1)[None, :]
        entries[key] = rows
    return hits


def memo_expected_hits_rows(snapshots, positions, n_mask, seed_len: int, mask_id: int, never=None) -> np.ndarray:
    """The rows memo's rule (option "memo_rows" of czc_generate_rows) stated on the host.  `snapshots` int32 [n_steps, R, T]: an
    option-OFF trajectory recorded with snapshot_every = 1; `positions` int [n_steps, R]: row r visits positions[s][r] at step
    s.  Returns bool [n_steps, R]: whether row r hits at step s (czc_memo_rows_stats counts their sum).

    The step groups are those of memo_expected_hits (n_mask is one value per step for all rows).  Row r's key at a group is
    (its position at every step of the group, the group's n_mask list); its entry sits in the slot (r, first position of the
    group), so a visit of that first position under another key replaces it.  Row r hits when its slot holds the same key
    and the masked row it held then equals the one it holds now.  A group with more than MEMO_SUB steps or one that does not
    start with n_mask >= 1 neither hits nor records; a group with a step in `never` (bool [n_steps]) records and does not
    hit.  With the reference's orders a first position always comes with the same key, and the rule is memo_expected_hits
    applied to every row with its own order."""
    snaps = np.asarray(snapshots)
    n_steps, R, T = snaps.shape
    pos = np.asarray(positions).reshape(n_steps, R)
    nm = [1] * n_steps if n_mask is None else [int(x) for x in n_mask]
    never = np.zeros(n_steps, bool) if never is None else np.asarray(never, bool)
    hits = np.zeros((n_steps, R), bool)
    slots = [dict() for _ in range(R)]   # per row: first position -> (key, masked row)
    for s, g in memo_groups(nm, n_steps):
        if nm[s] < 1 or nm[s] > T or g > MEMO_SUB:
            continue
        hittable = not never[s:s + g].any()
        for r in range(R):
            key = tuple((int(pos[s + j, r]), nm[s + j]) for j in range(g))
            row = snaps[s, r].copy()   # the row the step left, masked again, is the row it saw
            c0 = seed_len + int(pos[s, r])
            row[c0:min(c0 + nm[s], T)] = mask_id
            prev = slots[r].get(key[0][0])
            if hittable and prev is not None and prev[0] == key and np.array_equal(prev[1], row):
                hits[s:s + g, r] = True
            slots[r][key[0][0]] = (key, row)
    return hits


def converging_setup(B: int = 16, L: int = 6, precision: int = native.PREC_BF16, n_hot: int = 150, seed: int = 0,
                     alpha: float = 0.02, beta: float = 2.0, logit_scale: float = 4.6052, flat_top: int = 8):
    """Full-size towers with a trained-like MLM head (`n_hot` regular tokens 5.6..16 logit units above a bulk that softmax(logits /
    0.1) sends to zero, tests/test_step_gpu.py::_peaky_bert_weights), the first `flat_top` of them level at the top so that the
    CLIP term (published logit scale x100 by default) chooses among them image by image.  The fluency term keeps the choice
    to a few words: at B = 16, L = 6 every image still moves in sweep 2, about half have reached a fixed point of the polishing
    sweep during sweep 3, nearly all by sweep 4 -- the step memo's ground, with partly converged batches on the way (flat_top = 0:
    every image settles in sweep 2).  Returns (setup, image embeds [B, 512], hyper, init row, seed_len)."""
    bcfg = synth.bert_base()
    w = synth.make_bert_weights(bcfg, 11)
    sv = cached_vocab(False)
    regular = np.nonzero(synth.make_token_mask(sv, regular_only=True)[0] > 0)[0]
    hot = np.random.default_rng(5).choice(regular, size=n_hot, replace=False)
    bias = w["cls.predictions.bias"].copy()
    lift = np.linspace(16.0, 5.6, n_hot).astype(np.float32)
    lift[:flat_top] = 16.0   # `flat_top` hot tokens share the top logit: the CLIP term picks among them, per image
    bias[hot] += lift
    w["cls.predictions.bias"] = bias
    if "cls.predictions.decoder.bias" in w:
        w["cls.predictions.decoder.bias"] = bias
    su = build_synthetic(False, precision, logit_scale=logit_scale, regular_only=True, bert_w=w, bert_cfg=bcfg)
    emb = np.random.default_rng(100 + seed).standard_normal((B, su.clip_cfg.proj)).astype(np.float32)
    su.engine.set_image_embeds(emb)
    prompt = "Image of a"
    init = np.array(su.bert_tok.encode(prompt + su.bert_tok.mask_token * L), dtype=np.int32)
    return su, emb, Engine.hyper(alpha, beta, 0.1), init, len(prompt.split()) + 1
