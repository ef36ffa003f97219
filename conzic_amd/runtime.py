"""Glue between the reference-shaped call surface (gen_utils / control_gen_utils / clip.clip at
the repo root) and the native engine: builds ONE engine per (masked-LM, CLIP, tokenizer) triple,
pulls weights from `state_dict()`, builds the device text-bridge tables from the two tokenizers,
and turns the reference's visiting orders into czc_generate step lists.

`model` may be a HF `BertForMaskedLM` (demo.py:125) or `conzic_amd.models.SyntheticLM`;
`clip` is `clip.clip.CLIP` (this repo's drop-in); `tokenizer` a HF `BertTokenizer` or
`conzic_amd.text.WordPieceTokenizer`.  There is no CPU fallback: without the HIP library or a GPU
`Engine(...)` raises `NativeError`.
"""
from __future__ import annotations

import math
import os
import random
import time
import weakref
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import native, synth
from .bridge import tables_from_tokenizers
from .engine import Engine
from .harness import order_positions, sample_schedules

# bf16 CLIP towers carry a cosine error of up to ~4e-3; clip/clip.py:95-98 multiplies the cosine by
# logit_scale.exp() ahead of softmax_K, so the fused score stays inside the 1e-3 budget only while that factor is
# small (measured on the full-size goldens: in budget at 14.3 = HF init, far out at 100 = published checkpoint).
BF16_MAX_LOGIT_SCALE_EXP = 20.0
# single-pass fp16 towers (same speed as bf16, 11 significand bits): cosine error ~1.8e-4, fused score 5e-5 at x14.3 and
# 2.3e-3 at x100 (measured on the full-size goldens, linear in the scale) -- in budget up to about x40
FP16_MAX_LOGIT_SCALE_EXP = 40.0

_PRECISIONS = {"bf16": native.PREC_BF16, "f32": native.PREC_F32, "fp32": native.PREC_F32,
               "split": native.PREC_SPLIT, "split_fp16": native.PREC_SPLIT, "fp16": native.PREC_FP16, "f16": native.PREC_FP16,
               "refine": native.PREC_REFINE}


def choose_precision(logit_scale: Optional[float]) -> int:
    """Engine precision for a checkpoint: CZC_PRECISION (bf16 | fp16 | refine | split | f32) when set, else by the CLIP
    logit scale -- bf16 MFMA towers where exp(logit_scale) leaves their cosine error inside the 1e-3 fused-score
    budget (<= x20), single-pass fp16 towers up to x40, and above that -- the published checkpoints, x100 -- the
    screen-then-refine engine: every candidate through the single-pass fp16 text tower, the candidates that carry the
    softmax_K mass re-encoded by the split-fp16 tower (fused score inside 1e-3 on all K candidates, trajectories
    identical to the reference on the goldens, ~1.7x the all-split engine's throughput).  Unknown scale: all split-fp16."""
    p = os.environ.get("CZC_PRECISION", "auto").lower()
    if p != "auto":
        return _PRECISIONS[p]
    if logit_scale is None:
        return native.PREC_SPLIT
    if math.exp(float(logit_scale)) > FP16_MAX_LOGIT_SCALE_EXP:
        return native.PREC_REFINE
    if math.exp(float(logit_scale)) > BF16_MAX_LOGIT_SCALE_EXP:
        return native.PREC_FP16
    return native.PREC_BF16


def _logit_scale_of(clip) -> Optional[float]:
    try:
        v = clip.clip_state_dict()["logit_scale"]
        if hasattr(v, "detach"):
            v = v.detach().float().cpu().numpy()
        return float(np.asarray(v, dtype=np.float32).reshape(-1)[0])
    except (KeyError, AttributeError, TypeError, ValueError):
        return None


class _Entry:
    """One cached engine plus weak references to the objects it was built from: an entry is only ever returned
    for the very objects that built it (ids can be recycled after garbage collection), and it closes its engine
    when any of them dies."""

    def __init__(self, eng: Engine, objs):
        self.eng = eng
        self.refs = [weakref.ref(o) for o in objs]

    def matches(self, objs) -> bool:
        return len(objs) == len(self.refs) and all(r() is o for r, o in zip(self.refs, objs))


_ENGINES: Dict[tuple, _Entry] = {}


def _lookup(key, objs) -> Optional[Engine]:
    ent = _ENGINES.get(key)
    if ent is None:
        return None
    if ent.matches(objs):
        return ent.eng
    ent.eng.close()  # stale: the ids were re-used by new objects
    del _ENGINES[key]
    return None


def _store(key, eng: Engine, objs) -> None:
    _ENGINES[key] = _Entry(eng, objs)
    for o in objs:
        try:
            weakref.finalize(o, evict, key)
        except TypeError:
            pass


def evict(key=None) -> None:
    """Close cached engines (all of them when key is None) and release their device memory."""
    keys = list(_ENGINES) if key is None else [key]
    for k in keys:
        ent = _ENGINES.pop(k, None)
        if ent is not None:
            ent.eng.close()


def _to_numpy_state(sd) -> Dict[str, np.ndarray]:
    out = {}
    for k, v in sd.items():
        if hasattr(v, "detach"):
            v = v.detach().float().cpu().numpy()
        out[k] = np.asarray(v, dtype=np.float32)
    return out


def bert_cfg_of(model) -> synth.BertCfg:
    c = getattr(model, "czc_cfg", None)
    if c is not None:
        return c
    h = model.config  # HF BertConfig
    return synth.BertCfg(vocab=h.vocab_size, hidden=h.hidden_size, layers=h.num_hidden_layers,
                         heads=h.num_attention_heads, inter=h.intermediate_size, max_pos=h.max_position_embeddings,
                         eps=h.layer_norm_eps)


def clip_cfg_of(clip) -> synth.ClipCfg:
    c = getattr(clip, "czc_cfg", None)
    if c is not None:
        return c
    h = clip.model.config  # HF CLIPConfig
    t, v = h.text_config, h.vision_config
    return synth.ClipCfg(vocab=t.vocab_size, hidden=t.hidden_size, layers=t.num_hidden_layers,
                         heads=t.num_attention_heads, inter=t.intermediate_size, max_pos=t.max_position_embeddings,
                         eps=t.layer_norm_eps, proj=h.projection_dim, bos_id=clip.tokenizer.bos_token_id,
                         eos_id=clip.tokenizer.eos_token_id, v_hidden=v.hidden_size, v_layers=v.num_hidden_layers,
                         v_heads=v.num_attention_heads, v_inter=v.intermediate_size, v_image=v.image_size,
                         v_patch=v.patch_size)


def special_ids_of(tokenizer) -> Dict[str, int]:
    vocab = tokenizer.vocab if hasattr(tokenizer, "vocab") else tokenizer.get_vocab()
    return {k: int(vocab[k]) for k in ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", ".")}


PRECISION_NAMES = {native.PREC_BF16: "bf16", native.PREC_F32: "f32", native.PREC_SPLIT: "split-fp16", native.PREC_FP16: "fp16",
                   native.PREC_REFINE: "screen-then-refine (fp16 + split-fp16)", native.PREC_ALL_BF16: "all-bf16"}


def get_engine(model, clip, tokenizer, device: int = 0, precision: Optional[int] = None) -> Engine:
    """One engine per (model, clip, tokenizer, precision) on first use; precision None = `choose_precision`."""
    prec = choose_precision(_logit_scale_of(clip)) if precision is None else precision
    key = (id(model), id(clip), id(tokenizer), prec, device)
    objs = (model, clip, tokenizer)
    eng = _lookup(key, objs)
    if eng is None:
        bcfg, ccfg = bert_cfg_of(model), clip_cfg_of(clip)
        eng = Engine(bcfg, ccfg, special_ids_of(tokenizer), prec, device)
        eng.load_state(model.state_dict())
        eng.load_state(clip.clip_state_dict())
        eng.finalize()
        eng.set_bridge(tables_from_tokenizers(tokenizer, clip.tokenizer))
        if prec == native.PREC_REFINE and os.environ.get("CZC_REFINE_GUARD_X1E6"):
            eng.set_option("refine_guard_x1e6", int(os.environ["CZC_REFINE_GUARD_X1E6"]))  # trip point of the guard, 1e-6 of cosine
        _store(key, eng, objs)
    clip._engine = eng
    return eng


def clip_only_engine(clip, device: int = 0) -> Engine:
    """Engine without the BERT tower, for `CLIP.compute_*` calls made outside a generate call."""
    prec = choose_precision(_logit_scale_of(clip))
    key = (id(clip), "clip-only", prec, device)
    eng = _lookup(key, (clip,))
    if eng is None:
        eng = Engine(None, clip_cfg_of(clip), {}, prec, device)
        eng.load_state(clip.clip_state_dict())
        eng.finalize()
        _store(key, eng, (clip,))
    return eng


STREAMS_MIN_IMAGES = 32  # images per stream below which a batch is not split (smaller launches lose more than overlap gains)


def _group_for(eng: Engine, batch_size: int):
    """The engine itself, or its EngineGroup (engine + replicas on their own streams) when the batch is big enough
    for CZC_STREAMS (default 2) sub-batches of at least STREAMS_MIN_IMAGES images."""
    n = int(os.environ.get("CZC_STREAMS", "2"))
    if n <= 1 or batch_size < 2 * STREAMS_MIN_IMAGES:
        return eng
    grp = getattr(eng, "_group", None)
    if grp is None or grp.streams != n or grp.engines[0] is not eng or eng.h is None:
        from .engine import EngineGroup
        if grp is not None:
            grp.close(parent=False)
        grp = EngineGroup(eng, streams=n, min_images=STREAMS_MIN_IMAGES)
        eng._group = grp
    return grp


def advance_order_rng(order: str, max_len: int, max_iters: int) -> None:
    """Consume from the process-global RNG streams exactly what one *_generation call would (gen_utils.py:110-111
    shuffle: one `random.shuffle`; :210 random: one `np.random.randint` per iteration).  A rank of an image-sharded
    run calls this for the batches it does NOT own, so that every batch sees the visiting order it would have seen
    in the single-process run (SURVEY.md §8e parity caveat)."""
    if order == "shuffle":
        random.shuffle(list(range(max_len)))
    elif order == "random":
        for _ in range(max_iters):
            np.random.randint(0, max_len)


def _mask_to_numpy(token_mask) -> np.ndarray:
    if hasattr(token_mask, "detach"):
        return token_mask.detach().float().cpu().numpy()
    return np.asarray(token_mask, dtype=np.float32)


def memo_setting() -> int:
    """CZC_MEMO=0|1 (default 0): engine option "memo" of every generation call -- czc_generate runs a step only for the
    images whose masked row differs from their last visit of the same position in the call (exact: the others would get
    the same winner and cosine again; include/conzic_hip.h)."""
    v = os.environ.get("CZC_MEMO", "0").strip().lower()
    if v in ("0", "", "off", "false", "no"):
        return 0
    if v in ("1", "on", "true", "yes"):
        return 1
    raise ValueError(f"CZC_MEMO={v!r}: expected 0 or 1")


def memo_rows_setting() -> int:
    """CZC_MEMO_ROWS=0|1 (default 0): engine option "memo_rows" of the batched sample call (run_generation_samples) --
    czc_generate_rows runs a step only for the rows whose masked row differs from their last visit of the same position in
    the call (the rule of CZC_MEMO keyed per row; include/conzic_hip.h)."""
    v = os.environ.get("CZC_MEMO_ROWS", "0").strip().lower()
    if v in ("0", "", "off", "false", "no"):
        return 0
    if v in ("1", "on", "true", "yes"):
        return 1
    raise ValueError(f"CZC_MEMO_ROWS={v!r}: expected 0 or 1")


def _polish_guarded(polish, eng, model, clip, tokenizer, image_instance, logger):
    """`polish(engine) -> ((ids, cos), runner)` with what every generation call does around it: the overflow retry on fp32 rows
    and the screen-then-refine guard's rerun on the all-split engine."""
    try:
        (ids, cos), runner = polish(eng)
    except native.NativeError as exc:
        # the bf16 engine -- and, inside czc_generate, the screening pass of the screen-then-refine engine -- keep the text tower's
        # residual stream as fp16 rows (|x| < 65504): a checkpoint whose rows leave that range shows up as a non-finite cosine
        # (CZC_ERR_OVERFLOW); its engine then goes back to fp32 rows for good
        opt = {native.PREC_BF16: "resid16", native.PREC_REFINE: "refine_rows16"}.get(eng.precision)
        if getattr(exc, "code", None) != native.ERR_OVERFLOW or "non-finite" not in str(exc) or opt is None \
                or getattr(eng, "_resid16_off", False):
            raise   # (CZC_ERR_OVERFLOW also names the text bridge's scratch overflow: no other rows would help there)
        logger.info(f"the fp16 residual stream overflowed on this checkpoint; repeating the call with fp32 rows "
                    f"(engine option {opt} = 0, kept for this engine)")
        eng.set_option(opt, 0)
        eng._resid16_off = True
        (ids, cos), runner = polish(eng)
    guard_mode = os.environ.get("CZC_REFINE_GUARD", "rerun").lower()
    if eng.precision == native.PREC_REFINE and guard_mode != "off":
        # the screen-then-refine engine's 1e-3 bound rests on the single-pass fp16 tower's error staying near what it is
        # on the validated weights; every step measures that error on the candidates it re-encodes exactly
        g = runner.refine_guard(reset=True)
        if g["tripped"]:
            trip = eng.get_option("refine_guard_generate_x1e6") * 1e-6   # the trip point the engine applied inside czc_generate
            logger.info(f"screen-then-refine guard: |screening error - mean| reached {g['max_dev']:.2e} on {g['tripped']} "
                        f"image-steps (trip point {trip:.1e})" + ("; repeating the call on the all-split engine" if guard_mode == "rerun" else ""))
            if guard_mode == "rerun":
                from clip.clip import ImageEmbeds
                emb = image_instance.embeds if isinstance(image_instance, ImageEmbeds) else clip.last_image_embeds()
                # the replicas' workspaces (one per stream) go before the second engine is built on the same GPU
                grp = getattr(eng, "_group", None)
                if grp is not None:
                    grp.close(parent=False)
                    eng._group = None
                eng2 = get_engine(model, clip, tokenizer, precision=native.PREC_SPLIT)
                eng2.set_image_embeds(emb)   # the refine engine's vision tower is the split-fp16 one: same embeddings
                (ids, cos), _ = polish(eng2)
                clip._engine = eng
    return ids, cos


def _rival_call(rivals, delta, clip, image_instance, batch_size: int):
    """The rival table of a generation call, or None when the call has none (`rivals` None or `delta` 0).  `rivals`: an int M --
    every captioned image against its M nearest others among the resident images (conzic_amd.rivals.rival_table) -- or an int
    table [batch_size, M] of indices into the resident images (-1 = empty slot).  The resident images are those of
    `image_instance`: the first `batch_size` are captioned, any behind them serve as rivals only.
    Returns dict(table int32 [batch_size, M], delta, emb fp32 [n_images, proj])."""
    if rivals is None or not delta:
        return None
    if not math.isfinite(float(delta)):
        raise ValueError(f"delta = {delta!r} must be finite")
    from . import rivals as rv
    from clip.clip import ImageEmbeds
    emb = image_instance.embeds if isinstance(image_instance, ImageEmbeds) else clip.last_image_embeds()
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    if emb.shape[0] < batch_size:
        raise ValueError(f"{emb.shape[0]} resident images for a batch of {batch_size}")
    if isinstance(rivals, (int, np.integer)):
        if emb.shape[0] < 2:
            raise ValueError("rival images need at least two images in the batch")
        table = rv.rival_table(emb, min(int(rivals), emb.shape[0] - 1))[:batch_size]
    else:
        table = np.ascontiguousarray(rivals, dtype=np.int32)
    rv.check_table(table, np.arange(batch_size), emb.shape[0])
    return dict(table=table, delta=float(delta), emb=emb)


def _rival_engine(eng: Engine, vs, model, clip, tokenizer, logger) -> Engine:
    """The engine a call with rivals runs on: `eng`, unless that is the screen-then-refine engine, whose selection and guard
    bounds were derived for the softmax-K term alone (czc_generate_rows_vs refuses it) -- then the all-split engine, obtained the
    way the guard's rerun obtains it, holding the same image embeddings."""
    if vs is None or eng.precision != native.PREC_REFINE:
        return eng
    logger.info("rival images: the screen-then-refine engine's bounds do not cover the rival term; "
                "this call runs on the split-fp16 engine")
    grp = getattr(eng, "_group", None)
    if grp is not None:   # the replicas' workspaces go before the second engine is built on the same GPU
        grp.close(parent=False)
        eng._group = None
    eng2 = get_engine(model, clip, tokenizer, precision=native.PREC_SPLIT)
    eng2.set_image_embeds(vs["emb"])
    clip._engine = eng
    return eng2


def _log_own_probability(eng: Engine, vs, ids, seed_len: int, image_of_row, img_name, logger, what: str = "") -> None:
    """After the last sweep: P(own image | caption) among every image's rival set (czc_score_rows_vs), one line per row."""
    if vs is None or ids is None or not len(ids):
        return
    from . import rivals as rv
    ior = np.asarray(image_of_row, dtype=np.int32)
    eng.set_image_embeds(vs["emb"])
    _, disc = eng.score_rows_vs(np.ascontiguousarray(ids[-1], dtype=np.int32), seed_len, rv.expand(vs["table"], ior), None, ior)
    for r, b in enumerate(ior.tolist()):
        n = int((vs["table"][b] >= 0).sum())
        logger.info(f"{what}The {b + 1}-th image: {img_name[b]}, P(own image | caption) among {n + 1} images: {float(disc[r]):.3f}")


def caption_fluency(eng: Engine, ids, seed_len: int, lens, tokenizer, img_name, logger, what: str = ""):
    """After the last sweep: BERT's pseudo-log-likelihood of the final captions `ids` int [R, T] (czc_fluency_rows on `eng`; row r
    belongs to image r % len(img_name), the sample-major layout of the rows calls), one line per caption: PLL, mean log p,
    pseudo-perplexity and the word BERT ranks lowest.  Returns fluency.summarize's records, each with its `image` index added."""
    from . import fluency as fl
    rows = np.ascontiguousarray(ids, dtype=np.int32)
    if rows.ndim != 2 or not len(rows):
        return []
    res = eng.fluency_rows(rows, seed_len, lens=lens)
    recs = fl.summarize(res["logp"], res["rank"], lens)
    for r, rec in enumerate(recs):
        b = r % len(img_name)
        word = tokenizer.convert_ids_to_tokens([int(rows[r, seed_len + rec["worst_pos"]])])[0]
        rec["image"] = b
        logger.info(f"{what}The {b + 1}-th image: {img_name[b]}, fluency: PLL {rec['pll']:.4f}, mean log p {rec['mean_logp']:.4f}, "
                    f"pseudo-perplexity {rec['ppl']:.2f}, worst word '{word}' at position {rec['worst_pos']} (rank {rec['worst_rank']})")
    return recs


def _fluency_after(fluency, eng: Engine, ids, cos, seed_len: int, tokenizer, img_name, logger, sample0: int = 0) -> None:
    """`fluency` of the run_generation* functions: falsy = nothing; True = log caption_fluency of the last snapshot; a list =
    that, and every caption's record (with `sample`, `cos` = the final cosine and `ids` = the final row) is appended to it."""
    if fluency is None or fluency is False or ids is None or not len(ids):   # (an empty list is a collector: on)
        return
    recs = caption_fluency(eng, ids[-1], seed_len, None, tokenizer, img_name, logger)
    if isinstance(fluency, list):
        for r, rec in enumerate(recs):
            rec.update(sample=sample0 + r // len(img_name), cos=float(cos[-1][r]), ids=np.array(ids[-1][r], dtype=np.int32))
            fluency.append(rec)



def log_picked(logger, img_name, records, lam: float, tokenizer) -> list:
    """`--pick_lambda` of the CLIs: per image, the sample whose final caption has the largest cos + lam * mean log p among the
    records a `fluency` list collected (the first sample on ties); one "picked caption" line per image.  Returns, per image, the
    picked record (None for an image without records)."""
    from . import fluency as fl
    picked = []
    for b, name in enumerate(img_name):
        recs = sorted((r for r in records if r["image"] == b), key=lambda r: r["sample"])
        if not recs:
            picked.append(None)
            continue
        rec = recs[fl.pick([r["cos"] for r in recs], [r["mean_logp"] for r in recs], lam)]
        text = tokenizer.decode(rec["ids"].tolist(), skip_special_tokens=True)
        logger.info(f"The {b + 1}-th image: {name}, picked caption (sample {rec['sample']}, clip score {rec['cos']:.3f}, "
                    f"mean log p {rec['mean_logp']:.4f}, lambda {lam:g}): {text}")
        picked.append(rec)
    return picked


def _bookkeeping(order, ids, cos, tokenizer, img_name, logger, batch_size, verbose, print_every):
    """gen_utils.py:82-96 on the snapshots of one *_generation call: (gen_texts_list, clip_score_sequence)."""
    best_score = [0] * batch_size
    best_cap = ['None'] * batch_size
    texts_out, scores_out = [], []
    pe = print_every or 1
    for s in range(ids.shape[0]):
        cur = [float(x) for x in cos[s]]
        cur_text = tokenizer.batch_decode(ids[s].tolist(), skip_special_tokens=True)
        for jj in range(batch_size):
            if best_score[jj] < cur[jj]:
                best_score[jj] = cur[jj]
                best_cap[jj] = cur_text[jj]
        if order == "random" and not (verbose and (s + 1) % pe == 0):
            continue  # gen_utils.py:232-238: the random order only records a snapshot inside its verbose branch
        if verbose:
            for_print = tokenizer.batch_decode(ids[s].tolist())
            for jj in range(batch_size):
                logger.info(f"iter {s + 1}, The {jj + 1}-th image: {img_name[jj]},"
                            f"clip score {cur[jj]:.3f}: " + for_print[jj])
        texts_out.append(cur_text)
        scores_out.append(cur)
    texts_out.append(best_cap)
    scores_out.append(best_score)
    return texts_out, scores_out


def run_generation(order: str, img_name, model, clip, tokenizer, image_instance, token_mask, prompt, logger, max_len,
                   top_k, temperature, alpha, beta, max_iters, batch_size, verbose=True, gamma=None,
                   ctl_signal="positive", print_every: Optional[int] = None, pos_template=None, rivals=None, delta: float = 0.0,
                   fluency=False):
    """Body shared by every *_generation function (gen_utils.py:51-242, control_gen_utils.py:30-134):
    returns (gen_texts_list, clip_score_sequence) with the reference's list structure.
    `rivals` / `delta` (_rival_call): discriminative captions -- every candidate's fused score gets delta * P(own image |
    candidate) among the image and its rivals added (czc_generate_rows_vs: the batch as rows with the identity image map and the
    one shared order).  "best" is still chosen by cosine; after the last sweep P(own image | caption) is logged per image.
    `fluency` (_fluency_after): after the last sweep the final captions' BERT pseudo-log-likelihood is logged per image; it changes
    neither the captions nor what is returned."""
    import utils as ref_utils  # the repo-root drop-in (same functions as the reference's utils.py)
    eng = get_engine(model, clip, tokenizer)
    seed_len = len(prompt.split()) + 1                                   # gen_utils.py:56
    batch = ref_utils.get_init_text(tokenizer, prompt, max_len, batch_size)  # gen_utils.py:57
    clip.compute_image_representation_from_image_instance(image_instance)    # gen_utils.py:58 (cached in the engine)
    if getattr(eng, "_precision_logged", None) is None:
        scale = _logit_scale_of(clip)
        logger.info(f"engine precision: {PRECISION_NAMES.get(eng.precision, eng.precision)}"
                    + (f" (exp(logit_scale) = {math.exp(scale):.1f})" if scale is not None else ""))
        eng._precision_logged = True
    order_list = random_positions = None
    if order == "shuffle":
        order_list = list(range(max_len))
        random.shuffle(order_list)                                       # gen_utils.py:110-111 (process-global stream)
        logger.info(f"Order_list:{order_list}")
    elif order == "random":
        random_positions = [int(np.random.randint(0, max_len)) for _ in range(max_iters)]  # gen_utils.py:210
    iters = max_iters if order != "random" else max_iters // max_len
    if order == "random":
        positions, n_mask, every = [int(p) for p in random_positions], [1] * len(random_positions), 1
    else:
        positions, n_mask, every = order_positions(order, max_len, iters, order_list=order_list)
    hp = Engine.hyper(alpha, beta, temperature, gamma, ctl_signal == "negative",
                      control="pos" if pos_template is not None else None)
    vs = _rival_call(rivals, delta, clip, image_instance, batch_size)
    eng = _rival_engine(eng, vs, model, clip, tokenizer, logger)

    def polish(eng):
        """One whole *_generation call on `eng` (which must hold the batch's image embeddings)."""
        eng.set_token_mask(_mask_to_numpy(token_mask))
        eng.set_option("memo", memo_setting())  # exact step memo (CZC_MEMO); forwarded to the replicas of a group
        if gamma is not None:
            # control scores: caller-provided tables, else (default, CZC_CONTROL=auto) the reference's own sentence scorer
            # called back per step while the CLIP tower runs, else -- CZC_CONTROL=table -- tables built once per tokenizer
            # from nltk; raises without nltk and tables
            from . import control
            chosen = control.configure(eng, clip, tokenizer, pos_template=pos_template, ctl_signal=ctl_signal)
            if chosen != getattr(eng, "_control_logged", None):
                logger.info(f"control scores: {chosen}")
                eng._control_logged = chosen
        runner = _group_for(eng, batch_size)
        emb = None
        if runner is not eng:
            # two (CZC_STREAMS) contiguous image sub-batches on their own HIP streams over the same weights: the same
            # captions image for image (images are independent, gen_utils.py:64-81), their kernels overlap on the GPU
            from clip.clip import ImageEmbeds
            emb = image_instance.embeds if isinstance(image_instance, ImageEmbeds) else clip.last_image_embeds()
            runner.set_image_embeds(emb)
        if eng.precision == native.PREC_REFINE:
            runner.refine_guard(reset=True)
        if vs is not None:
            rows_pos = np.ascontiguousarray(np.repeat(np.asarray(positions, dtype=np.int32)[:, None], batch_size, axis=1))
            out = runner.generate_rows_vs(np.repeat(np.asarray(batch[0], dtype=np.int32)[None, :], batch_size, axis=0), None, seed_len,
                                          top_k, rows_pos, [hp] * batch_size, None, None, vs["table"], [vs["delta"]] * batch_size,
                                          image_of_row=np.arange(batch_size, dtype=np.int32), n_mask=n_mask, snapshot_every=every)
        else:
            out = runner.generate(batch_size, batch[0], max_len, seed_len, top_k, positions, hp, n_mask=n_mask,
                                  snapshot_every=every)
        if runner is not eng:
            eng.set_image_embeds(emb)  # the first engine holds the whole batch again, as after a single-stream call
        return out, runner

    ids, cos = _polish_guarded(polish, eng, model, clip, tokenizer, image_instance, logger)
    _log_own_probability(eng, vs, ids, seed_len, np.arange(batch_size), img_name, logger)
    _fluency_after(fluency, eng, ids, cos, seed_len, tokenizer, img_name, logger)
    # utils.update_token_mask mutates the caller's mask in place (utils.py:53-59): leave it as the
    # reference would after the last visited position
    if positions:
        ref_utils.update_token_mask(tokenizer, token_mask, max_len, positions[-1])
    return _bookkeeping(order, ids, cos, tokenizer, img_name, logger, batch_size, verbose, print_every)


def run_generation_samples(order: str, samples_num: int, img_name, model, clip, tokenizer, image_instance, token_mask, prompt,
                           logger, max_len, top_k, temperature, alpha, beta, max_iters, batch_size, verbose=True, gamma=None,
                           ctl_signal="positive", print_every: Optional[int] = None, pos_template=None, schedules=None,
                           sample_tau: float = 0.0, sample_seed: int = 0, sample0: int = 0, rivals=None, delta: float = 0.0,
                           fluency=False, vocab=None):
    """The sample loop around a *_generation call (demo.py:83, run.py) as ONE engine call: `samples_num` samples of a batch of
    `batch_size` images ride as batch_size * samples_num rows of czc_generate_rows, every sample with the visiting order the
    serial loop would have drawn for it (harness.sample_schedules); the images are encoded once.  Returns a list of
    `samples_num` (gen_texts_list, clip_score_sequence) pairs, the s-th as the s-th serial `run_generation` call returns it,
    and logs every sample's lines in the serial loop's order.  The reference's own sentence scorer (exact control mode) is
    told one position per step, so with orders that differ between samples the engine is called once per sample, as the serial
    loop calls it (same orders, same results, the images still encoded once), and the log says why.
    `schedules`: what harness.sample_schedules returned for these samples when the caller drew the orders itself (run_cli draws
    those of all batches first, in the serial loop's sample-major order); None: drawn here.
    `sample_tau` > 0: every row draws its winner from softmax_K(final_score / sample_tau) (czc_generate_rows_draw) under the
    seed of its (image, sample): draws.row_seed(sample_seed, key of the image's name, sample0 + s).  A serial loop that calls
    this function once per sample (samples_num = 1, sample0 = the sample's index) returns the ids of the one batched call.
    `rivals` / `delta`: as for run_generation; every sample of an image carries the image's rivals (czc_generate_rows_vs).
    `fluency`: as for run_generation, one line per (sample, image) row.
    `vocab`: a vocab.Vocab, or bitsets uint32 [W] / [n, W] (vocab.pack): one vocabulary set for every row, or one per sample
    (n = the samples of the whole loop; sample sample0 + s takes set sample0 + s), applied on top of the token mask
    (czc_generate_rows_vocab).  An allow-list that leaves fewer than top_k ids after the token mask is refused (ValueError)."""
    from . import draws as dw
    from . import vocab as vc
    import utils as ref_utils
    S, B = int(samples_num), int(batch_size)
    if vocab is not None and not isinstance(vocab, vc.Vocab):
        vocab = vc.Vocab(vocab)
    if vocab is not None:   # before any engine work: the sets' sizes, and the refusal of an allow-list shorter than a step's K
        vocab.check(_mask_to_numpy(token_mask), top_k)
        set_of_sample = vocab.set_of_sample(S, sample0)
        vocab_said = vocab.describe(_mask_to_numpy(token_mask))
    eng = get_engine(model, clip, tokenizer)
    seed_len = len(prompt.split()) + 1
    batch = ref_utils.get_init_text(tokenizer, prompt, max_len, B)
    clip.compute_image_representation_from_image_instance(image_instance)   # once per image, not once per sample
    if getattr(eng, "_precision_logged", None) is None:
        scale = _logit_scale_of(clip)
        logger.info(f"engine precision: {PRECISION_NAMES.get(eng.precision, eng.precision)}"
                    + (f" (exp(logit_scale) = {math.exp(scale):.1f})" if scale is not None else ""))
        eng._precision_logged = True
    positions, n_mask, every, order_lists = schedules if schedules is not None else sample_schedules(order, max_len, max_iters, S)
    positions = np.asarray(positions, dtype=np.int32)
    assert positions.ndim == 2 and positions.shape[1] == S, positions.shape
    rows_pos = np.ascontiguousarray(np.repeat(positions, B, axis=1))   # row s * B + b: sample s of image b
    image_of_row = np.tile(np.arange(B, dtype=np.int32), S)
    orders_differ = bool((positions != positions[:, :1]).any())
    hp = Engine.hyper(alpha, beta, temperature, gamma, ctl_signal == "negative",
                      control="pos" if pos_template is not None else None)
    row_draws = dw.sample_rows(sample_seed, [dw.image_key(n) for n in img_name], S, float(sample_tau or 0.0), sample0=sample0)
    init_row = np.asarray(batch[0], dtype=np.int32)
    vs = _rival_call(rivals, delta, clip, image_instance, B)
    eng = _rival_engine(eng, vs, model, clip, tokenizer, logger)

    def vocab_rows(runner, s0, n_samples, pos_rows, draws_):
        """samples s0 .. s0 + n_samples - 1 of the batch as rows of one vocabulary call: sample-major, every row with its
        sample's set and, with rivals, its image's rivals"""
        from . import rivals as rv
        n = B * n_samples
        ior = np.tile(np.arange(B, dtype=np.int32), n_samples)
        return runner.generate_rows_vocab(np.repeat(init_row[None, :], n, axis=0), None, seed_len, top_k, pos_rows, [hp] * n, draws_, None,
                                          None if vs is None else rv.expand(vs["table"], ior), None if vs is None else [vs["delta"]] * n,
                                          sets=vocab.bits, set_of_row=np.repeat(set_of_sample[s0:s0 + n_samples], B),
                                          image_of_row=ior, n_mask=n_mask, snapshot_every=every)

    def vs_rows(runner, n_samples, pos_rows, draws_):
        """`n_samples` samples of the batch as rows of one rivals call: sample-major, every row with its image's rivals."""
        from . import rivals as rv
        ior = np.tile(np.arange(B, dtype=np.int32), n_samples)
        return runner.generate_rows_vs(np.repeat(init_row[None, :], B * n_samples, axis=0), None, seed_len, top_k, pos_rows,
                                       [hp] * (B * n_samples), draws_, None, rv.expand(vs["table"], ior),
                                       [vs["delta"]] * (B * n_samples), image_of_row=ior, n_mask=n_mask, snapshot_every=every)

    def polish(eng):
        eng.set_token_mask(_mask_to_numpy(token_mask))
        eng.set_option("memo", memo_setting())  # for the one-call-per-sample arm below; a rows call ignores it
        eng.set_option("memo_rows", memo_rows_setting())  # per-row step memo of the rows call (CZC_MEMO_ROWS)
        chosen = None
        if gamma is not None:
            from . import control
            chosen = control.configure(eng, clip, tokenizer, pos_template=pos_template, ctl_signal=ctl_signal)
            if chosen != getattr(eng, "_control_logged", None):
                logger.info(f"control scores: {chosen}")
                eng._control_logged = chosen
        # the exact control scorer (a callback with ONE gen_idx per step) cannot serve rows at different positions
        one_by_one = gamma is not None and chosen == "exact" and orders_differ
        if one_by_one and not getattr(eng, "_one_by_one_logged", False):
            logger.info("batched samples: the exact control scorer is called with one position per step and the samples' "
                        f"{order} orders differ; running the {S} samples one call at a time (CZC_CONTROL=table batches them)")
            eng._one_by_one_logged = True
        runner = _group_for(eng, B if one_by_one else B * S)
        emb = None
        if runner is not eng:
            from clip.clip import ImageEmbeds
            emb = image_instance.embeds if isinstance(image_instance, ImageEmbeds) else clip.last_image_embeds()
            runner.set_image_embeds(emb)
        if eng.precision == native.PREC_REFINE:
            runner.refine_guard(reset=True)
        if vocab is not None and one_by_one:
            outs = [vocab_rows(runner, s, 1, np.ascontiguousarray(np.repeat(positions[:, s:s + 1], B, axis=1)),
                               None if row_draws is None else row_draws[s * B:(s + 1) * B]) for s in range(S)]
            out = tuple(np.concatenate([o[j] for o in outs], axis=1) for j in (0, 1))
        elif vocab is not None:
            out = vocab_rows(runner, 0, S, rows_pos, row_draws)
        elif vs is not None and one_by_one:
            outs = [vs_rows(runner, 1, np.ascontiguousarray(np.repeat(positions[:, s:s + 1], B, axis=1)),
                            None if row_draws is None else row_draws[s * B:(s + 1) * B]) for s in range(S)]
            out = tuple(np.concatenate([o[j] for o in outs], axis=1) for j in (0, 1))
        elif vs is not None:
            out = vs_rows(runner, S, rows_pos, row_draws)
        elif one_by_one and row_draws is not None:
            outs = [runner.generate_rows_draw(np.repeat(init_row[None, :], B, axis=0), None, seed_len, top_k,
                                              np.repeat(positions[:, s:s + 1], B, axis=1), [hp] * B, row_draws[s * B:(s + 1) * B],
                                              n_mask=n_mask, snapshot_every=every) for s in range(S)]
            out = tuple(np.concatenate([o[j] for o in outs], axis=1) for j in (0, 1))
        elif one_by_one:
            outs = [runner.generate(B, batch[0], max_len, seed_len, top_k, positions[:, s].tolist(), hp, n_mask=n_mask,
                                    snapshot_every=every) for s in range(S)]
            out = tuple(np.concatenate([o[j] for o in outs], axis=1) for j in (0, 1))
        elif row_draws is not None:
            out = runner.generate_rows_draw(np.repeat(init_row[None, :], B * S, axis=0), None, seed_len, top_k, rows_pos, [hp] * (B * S),
                                            row_draws, image_of_row=image_of_row, n_mask=n_mask, snapshot_every=every)
        else:
            out = runner.generate_rows(batch[0], max_len, seed_len, top_k, rows_pos, hp, image_of_row=image_of_row,
                                       n_mask=n_mask, snapshot_every=every)
        if runner is not eng:
            eng.set_image_embeds(emb)
        return out, runner

    ids, cos = _polish_guarded(polish, eng, model, clip, tokenizer, image_instance, logger)
    _log_own_probability(eng, vs, ids, seed_len, image_of_row, img_name, logger)
    _fluency_after(fluency, eng, ids, cos, seed_len, tokenizer, img_name, logger, sample0=sample0)
    if positions.shape[0]:   # the caller's mask as after the LAST sample's last position (utils.py:53-59)
        ref_utils.update_token_mask(tokenizer, token_mask, max_len, int(positions[-1, S - 1]))
    out = []
    for s in range(S):
        said = dw.describe(row_draws[s * B:(s + 1) * B] if row_draws else None)
        if vocab is not None:
            said += vocab_said + f" (sample {sample0 + s}: set {int(set_of_sample[s])})"
        if order_lists is not None:
            logger.info(f"Order_list:{order_lists[s]}" + said)
        elif said:
            logger.info(f"Order:{order}" + said)
        out.append(_bookkeeping(order, ids[:, s * B:(s + 1) * B], cos[:, s * B:(s + 1) * B], tokenizer, img_name, logger, B,
                                verbose, print_every))
    return out


def run_generation_lengths(order: str, lens: Sequence[int], samples_num: int, img_name, model, clip, tokenizer, image_instance,
                           token_mask, prompt, logger, top_k, temperature, alpha, beta, max_iters, batch_size, verbose=True,
                           gamma=None, ctl_signal="positive", pos_template=None, sample_tau: float = 0.0, sample_seed: int = 0,
                           sample0: int = 0, column0: int = 0):
    """The loop over sentence lengths around the sample loop (one CLI run per --sentence_len) as ONE engine call: `samples_num`
    samples at each length of `lens` of a batch of `batch_size` images ride as len(lens) * samples_num * batch_size rows of
    czc_generate_rows_len, row (l * samples_num + s) * batch_size + b = sample s at lens[l] of image b, at its own length
    (lengths.length_rows: no row reads another's padding) and with the visiting order the serial loop -- lengths outside, samples
    inside -- would have drawn for it (lengths.length_schedules: one draw per length and sample from the process-global stream);
    the images are encoded once.  `order` is sequential or shuffle, `max_iters` the number of sweeps.  Returns, per length, a list
    of `samples_num` (gen_texts_list, clip_score_sequence) pairs, each as the `run_generation` call at that length returns it, and
    logs every call's lines in the serial loop's order.  The reference's own sentence scorer (exact control mode) is told one
    position and one row length per step: with it the engine is called once per length and sample, as the serial loop calls it
    (same orders, same results, the images still encoded once), and the log says why.
    `sample_tau` > 0: every row draws its winner (czc_generate_rows_draw) under draws.row_seed(sample_seed, key of the image's
    name, sample0 + s, column0 + l); a row's step counter is its step in the call at hand."""
    import utils as ref_utils
    from . import draws as dw, lengths
    lens = [int(n) for n in lens]
    S, B, NL = int(samples_num), int(batch_size), len(lens)
    if S < 1 or B < 1:
        raise ValueError(f"run_generation_lengths: samples_num = {S} and batch_size = {B} must be >= 1")
    seed_len = len(prompt.split()) + 1
    col_lens = [n for n in lens for _ in range(S)]                            # column l * S + s: sample s at lens[l]
    positions, n_mask, every = lengths.length_schedules(col_lens, order, max_iters)   # (validates lens and order, draws the orders)
    eng = get_engine(model, clip, tokenizer)
    clip.compute_image_representation_from_image_instance(image_instance)   # once per image, whatever the lengths and samples
    if getattr(eng, "_precision_logged", None) is None:
        scale = _logit_scale_of(clip)
        logger.info(f"engine precision: {PRECISION_NAMES.get(eng.precision, eng.precision)}"
                    + (f" (exp(logit_scale) = {math.exp(scale):.1f})" if scale is not None else ""))
        eng._precision_logged = True
    col_rows = lengths.length_rows(tokenizer, prompt, col_lens)
    init_rows = np.ascontiguousarray(np.repeat(col_rows, B, axis=0))
    row_lens = np.repeat(np.asarray(col_lens, dtype=np.int32), B)
    rows_pos = np.ascontiguousarray(np.repeat(positions, B, axis=1))
    image_of_row = np.tile(np.arange(B, dtype=np.int32), NL * S)
    T = init_rows.shape[1]
    hp = Engine.hyper(alpha, beta, temperature, gamma, ctl_signal == "negative",
                      control="pos" if pos_template is not None else None)
    row_draws = dw.sample_rows(sample_seed, [dw.image_key(n) for n in img_name], S, float(sample_tau or 0.0), columns=NL,
                               sample0=sample0, column0=column0)

    def polish(eng):
        eng.set_token_mask(_mask_to_numpy(token_mask))
        eng.set_option("memo", memo_setting())  # for the one-call-per-sample arm below; a rows call ignores it
        eng.set_option("memo_rows", memo_rows_setting())  # per-row step memo of the rows call (CZC_MEMO_ROWS)
        chosen = None
        if gamma is not None:
            from . import control
            chosen = control.configure(eng, clip, tokenizer, pos_template=pos_template, ctl_signal=ctl_signal)
            if chosen != getattr(eng, "_control_logged", None):
                logger.info(f"control scores: {chosen}")
                eng._control_logged = chosen
        # the exact control scorer (a callback with ONE gen_idx and ONE row length per step) cannot serve mixed rows
        one_by_one = gamma is not None and chosen == "exact" and (len(set(lens)) > 1 or bool((positions != positions[:, :1]).any()))
        if one_by_one and not getattr(eng, "_one_by_one_lengths_logged", False):
            logger.info("sentence lengths: the exact control scorer is called with one position and one length per step; running "
                        f"the {NL * S} length/sample pairs one call at a time (CZC_CONTROL=table batches them)")
            eng._one_by_one_lengths_logged = True
        runner = _group_for(eng, B if one_by_one else B * S * NL)
        emb = None
        if runner is not eng:
            from clip.clip import ImageEmbeds
            emb = image_instance.embeds if isinstance(image_instance, ImageEmbeds) else clip.last_image_embeds()
            runner.set_image_embeds(emb)
        if eng.precision == native.PREC_REFINE:
            runner.refine_guard(reset=True)
        if one_by_one:
            ids = np.zeros((max_iters, NL * S * B, T), dtype=np.int32)
            cos = np.zeros((max_iters, NL * S * B), dtype=np.float32)
            for c, n in enumerate(col_lens):
                own = positions.reshape(max_iters, every, NL * S)[:, :n, c].reshape(-1).tolist()   # the column without its idle steps
                if row_draws is not None:
                    i1, c1 = runner.generate_rows_draw(np.repeat(col_rows[c:c + 1, :seed_len + n + 1], B, axis=0), None, seed_len, top_k,
                                                       np.repeat(np.asarray(own, dtype=np.int32)[:, None], B, axis=1), [hp] * B,
                                                       row_draws[c * B:(c + 1) * B], snapshot_every=n)
                else:
                    i1, c1 = runner.generate(B, col_rows[c, :seed_len + n + 1].tolist(), n, seed_len, top_k, own, hp, snapshot_every=n)
                ids[:, c * B:(c + 1) * B, :seed_len + n + 1], cos[:, c * B:(c + 1) * B] = i1, c1
            out = (ids, cos)
        elif row_draws is not None:
            out = runner.generate_rows_draw(init_rows, row_lens, seed_len, top_k, rows_pos, [hp] * len(row_lens), row_draws,
                                            image_of_row=image_of_row, n_mask=n_mask, snapshot_every=every)
        else:
            out = runner.generate_rows_len(init_rows, row_lens, seed_len, top_k, rows_pos, hp, image_of_row=image_of_row,
                                           n_mask=n_mask, snapshot_every=every)
        if runner is not eng:
            eng.set_image_embeds(emb)
        return out, runner

    ids, cos = _polish_guarded(polish, eng, model, clip, tokenizer, image_instance, logger)
    if positions.shape[0]:   # the caller's mask as after the LAST call's last position: the last sample at the last length
        n = col_lens[-1]
        ref_utils.update_token_mask(tokenizer, token_mask, n, int(positions[(max_iters - 1) * every + n - 1, -1]))
    out = []
    for l, n in enumerate(lens):
        per_sample = []
        for s in range(S):
            c = l * S + s
            said = dw.describe(row_draws[c * B:(c + 1) * B] if row_draws else None)
            if order == "shuffle":
                logger.info(f"Order_list:{[int(p) for p in positions[:n, c]]}" + said)
            elif said:
                logger.info(f"Order:{order}" + said)
            per_sample.append(_bookkeeping(order, ids[:, c * B:(c + 1) * B, :seed_len + n + 1], cos[:, c * B:(c + 1) * B], tokenizer,
                                           img_name, logger, B, verbose, None))
        out.append(per_sample)
    return out


def run_infill(captions: Sequence[str], img_name, model, clip, tokenizer, image_instance, token_mask, prompt, logger, *,
               order: str = "sequential", max_iters: int = 10, top_k: int = 200, temperature=0.1, alpha=0.02, beta=2.0,
               positions: str = "blanks", image_of_caption: Optional[Sequence[int]] = None, blank: str = "_", verbose=True,
               sample_tau: float = 0.0, sample_seed: int = 0):
    """Infilling, resume and draft polishing (beyond the reference's CLI; its loop body, gen_utils.py:64-81, unchanged): every
    caption of `captions` is a template whose `blank` words are polished while the given words stay as context
    (`positions="blanks"`), or a draft / earlier result of which every position is polished again (`positions="all"`: nothing is
    idle).  Caption i describes image image_of_caption[i] of `image_instance` (None: caption i = image i, or all captions the
    one image).  The images are encoded once and all captions, whatever their token lengths, are the rows of ONE
    czc_generate_rows_len call, each at its own length (a shorter caption's padding is never read) with its own start row and
    visiting order (infill.infill_schedules, drawn in caption order), a caption with fewer blanks sitting out the rest of every
    sweep.  Logs, results and the token mask keep the order of infill.group_by_length (captions of one token length together,
    lengths in order of first appearance).  `max_iters` sweeps; honours CZC_MEMO_ROWS.  Returns one (gen_texts_list, clip_score_sequence) pair per caption, in the
    structure a *_generation call returns for a batch of one.  The caller's token_mask is left as after the last visited
    position (utils.py:53-59).  `sample_tau` > 0: caption i draws its winners (czc_generate_rows_draw) under
    draws.row_seed(sample_seed, key of its image's name, 0, i)."""
    import utils as ref_utils
    from . import draws as dw, infill
    captions = list(captions)
    if not captions:
        return []
    eng = get_engine(model, clip, tokenizer)
    clip.compute_image_representation_from_image_instance(image_instance)   # once, whatever the number of groups
    from clip.clip import ImageEmbeds
    emb = image_instance.embeds if isinstance(image_instance, ImageEmbeds) else clip.last_image_embeds()
    n_img = int(emb.shape[0])
    if image_of_caption is None:
        if n_img not in (1, len(captions)):
            raise ValueError(f"run_infill: {len(captions)} captions for {n_img} images need image_of_caption")
        image_of_caption = [0] * len(captions) if n_img == 1 else list(range(len(captions)))
    ioc = [int(i) for i in image_of_caption]
    if len(ioc) != len(captions) or any(i < 0 or i >= n_img for i in ioc):
        raise ValueError("run_infill: image_of_caption must name one resident image per caption")
    if getattr(eng, "_precision_logged", None) is None:
        scale = _logit_scale_of(clip)
        logger.info(f"engine precision: {PRECISION_NAMES.get(eng.precision, eng.precision)}"
                    + (f" (exp(logit_scale) = {math.exp(scale):.1f})" if scale is not None else ""))
        eng._precision_logged = True
    parsed = [infill.parse_template(tokenizer, prompt, c, blank=blank) for c in captions]
    visits = infill.visit_lists(parsed, positions)
    (T, members), = infill.group_for_call(parsed).items()   # every caption, in caption order: one call
    # one draw per caption from the process-global stream for `shuffle`, in caption order
    pos_all, n_mask, every = infill.infill_schedules(visits, order, max_iters)
    row_draws = None
    if sample_tau:
        row_draws = [dw.make_draw(dw.row_seed(sample_seed, dw.image_key(img_name[ioc[i]]), 0, i), sample_tau) for i in range(len(captions))]
    for i, v in enumerate(visits):
        said = dw.describe(row_draws[i:i + 1] if row_draws else None)
        if order == "shuffle":
            logger.info(f"Order_list:{[int(p) for p in pos_all[:len(v), i]]}" + said)
        elif said:
            logger.info(f"Order:{order}" + said)
    hp = Engine.hyper(alpha, beta, temperature)
    seed_len = parsed[0][3]
    init_rows = np.zeros((len(members), T), dtype=np.int32)   # id 0 ([PAD]) behind a shorter caption's [SEP]
    for i in members:
        init_rows[i, :parsed[i][0].size] = parsed[i][0]
    row_lens = np.asarray([parsed[i][2] for i in members], dtype=np.int32)
    image_of_row = np.asarray(ioc, dtype=np.int32)

    def polish(eng):
        eng.set_token_mask(_mask_to_numpy(token_mask))
        eng.set_option("memo_rows", memo_rows_setting())  # per-row step memo (CZC_MEMO_ROWS); an idle step is not a visit
        runner = _group_for(eng, len(members))
        if runner is not eng:
            runner.set_image_embeds(emb)
        if eng.precision == native.PREC_REFINE:
            runner.refine_guard(reset=True)
        if row_draws is not None:
            res = runner.generate_rows_draw(init_rows, row_lens, seed_len, top_k, pos_all, [hp] * len(members), row_draws,
                                            image_of_row=image_of_row, n_mask=n_mask, snapshot_every=every)
        elif int(row_lens.min()) == int(row_lens.max()):   # one token length: czc_generate_rows_from, as before there were lengths
            res = runner.generate_rows_from(init_rows, int(row_lens[0]), seed_len, top_k, pos_all, hp, image_of_row=image_of_row,
                                            n_mask=n_mask, snapshot_every=every)
        else:
            res = runner.generate_rows_len(init_rows, row_lens, seed_len, top_k, pos_all, hp, image_of_row=image_of_row,
                                           n_mask=n_mask, snapshot_every=every)
        if runner is not eng:
            eng.set_image_embeds(emb)
        return res, runner

    ids, cos = _polish_guarded(polish, eng, model, clip, tokenizer, ImageEmbeds(emb), logger)
    out = [None] * len(captions)
    last = None
    for same_len in infill.group_by_length(parsed).values():   # the order of the logs and of the mask's last visit
        lv = infill.last_visited(pos_all[:, same_len])
        if lv is not None:
            last = (parsed[same_len[0]][2], lv)
        for i in same_len:
            out[i] = _bookkeeping(order, ids[:, i:i + 1, :parsed[i][0].size], cos[:, i:i + 1], tokenizer, [img_name[ioc[i]]], logger,
                                  1, verbose, None)
    if last is not None:
        ref_utils.update_token_mask(tokenizer, token_mask, last[0], last[1])
    return out


def infill_captions(captions, img_name, model, clip, tokenizer, image_instance, token_mask, logger, *, prompt="", top_k=100,
                    temperature=1.0, max_iter=10, alpha=0.7, beta=1, generate_order="sequential", positions="blanks",
                    image_of_caption=None, sample_tau=0.0, sample_seed=0):
    """`--run_type infill` of the two CLIs: one run_infill call over the `--caption` templates, logging every caption's final
    and best text as generate_caption does (gen_utils.py:325-331)."""
    start_time = time.time()
    order = "sequential" if generate_order == "sequential" else "shuffle"
    outs = run_infill(captions, img_name, model, clip, tokenizer, image_instance, token_mask, prompt, logger, order=order,
                      max_iters=max_iter, top_k=top_k, temperature=temperature, alpha=alpha, beta=beta, positions=positions,
                      image_of_caption=image_of_caption, sample_tau=sample_tau, sample_seed=sample_seed)
    logger.info("Finished in %.3fs" % (time.time() - start_time))
    for i, (generate_texts, _) in enumerate(outs):
        logger.info(f"The {i + 1}-th caption: {captions[i]}")
        logger.info(f"final caption: {generate_texts[-2][0] if len(generate_texts) > 1 else 'None'}")
        logger.info(f"best caption: {generate_texts[-1][0]}")
    return outs


def caption_order(run_type: str, generate_order: str, ctl_type: str, max_iter: int, max_len: int):
    """(visiting order, max_iters) the *_generation function behind generate_caption / control_generate_caption runs with."""
    if run_type == "caption":
        return generate_order, (max_iter * max_len if generate_order == "random" else max_iter)   # gen_utils.py:305-306
    if ctl_type == "sentiment":
        return ("sequential" if generate_order == "sequential" else "shuffle"), max_iter         # control_gen_utils.py:205-217
    return "sequential", max_iter                                                                 # control_gen_utils.py:218-223


def caption_samples(samples_num: int, run_type: str, img_name, model, clip, tokenizer, image_instance, token_mask, logger, *,
                    prompt="", batch_size=1, max_len=15, top_k=100, temperature=1.0, max_iter=500, alpha=0.7, beta=1,
                    generate_order="sequential", gamma=5, ctl_type="sentiment", style_type="positive", pos_type=None,
                    schedules=None, sample_tau=0.0, sample_seed=0, sample0=0, rivals=None, delta=0.0, fluency=False, vocab=None):
    """`--batch_samples` of the two CLIs: what `samples_num` calls of generate_caption (run_type 'caption', gen_utils.py:289-333)
    or control_generate_caption (control_gen_utils.py:197-232) return, from one run_generation_samples call.  Returns the list
    of (generate_texts, clip_scores) pairs and logs every sample's final and best captions as those functions do."""
    start_time = time.time()
    kw = dict(verbose=True)
    if run_type == "caption" and generate_order not in ("sequential", "shuffle", "span", "random"):
        raise ValueError(f"generate_order must be sequential|shuffle|random|span, got {generate_order!r}")
    order, max_iters = caption_order(run_type, generate_order, ctl_type, max_iter, max_len)
    if run_type == "caption":
        if order == "random":
            kw["print_every"] = max_len
    elif ctl_type == "sentiment":
        kw.update(gamma=gamma, ctl_signal=style_type)
    else:
        logger.info(pos_type)
        kw.update(gamma=gamma, pos_template=pos_type)
    outs = run_generation_samples(order, samples_num, img_name, model, clip, tokenizer, image_instance, token_mask, prompt,
                                  logger, max_len, top_k, temperature, alpha, beta, max_iters, batch_size, schedules=schedules,
                                  sample_tau=sample_tau, sample_seed=sample_seed, sample0=sample0, rivals=rivals, delta=delta,
                                  fluency=fluency, vocab=vocab, **kw)
    logger.info("Finished %d samples in %.3fs" % (samples_num, time.time() - start_time))
    for sample_id, (generate_texts, _) in enumerate(outs):
        logger.info(f"Sample {sample0 + sample_id}: ")
        for i in range(batch_size):
            logger.info(f"The {i + 1}-th image: {img_name[i]}")
            logger.info(f"final caption: {generate_texts[-2][i]}")
            logger.info(f"best caption: {generate_texts[-1][i]}")
    return outs


def run_generation_blocks(order: str, width: int, layout: str, samples_num: int, img_name, model, clip, tokenizer, image_instance,
                          token_mask, prompt, logger, max_len, top_k, temperature, alpha, beta, max_iters, batch_size,
                          verbose=True, gamma=None, ctl_signal="positive", print_every: Optional[int] = None, pos_template=None,
                          sample_tau: float = 0.0, sample_seed: int = 0, sample0: int = 0):
    """Block-synchronous sweeps (czc_generate_rows_tied, conzic_amd/blocks.py): every caption is polished by `width` tied rows
    that each mask, propose and score one position of the step's block from the same current sentence; all winners are written
    back together.  A sweep costs ceil(max_len / width) serial steps instead of max_len, each on a batch `width` times larger.
    Rows are images x samples x width: row ((s * B + b) * width + slot), one engine call for all of them.
    `order` sequential: the blocks of blocks.sequential_order under `layout` (interleaved | contiguous).  shuffle: every
    sample's permutation is drawn exactly as run_generation draws it (one `random.shuffle` per sample from the process-global
    stream, the same list every sweep) and cut into consecutive blocks; `layout` does not apply.  span / random: ValueError.
    width 0 means max_len; width 1 is run_generation_samples itself.  The exact host control scorer (a callback told one
    position per step) cannot serve a block: such a run falls back to width 1 and the log says so.
    `sample_tau` > 0: slot j of (image, sample) draws under draws.row_seed(sample_seed, key of the image's name, sample, j).
    Returns a list of `samples_num` (gen_texts_list, clip_score_sequence) pairs in run_generation's structure -- texts per sweep
    plus best, cosines per sweep plus best -- where the cosines are those of the merged captions (czc_score_rows) and "best"
    is chosen by them."""
    from . import blocks as bl, draws as dw
    import utils as ref_utils
    if order not in ("sequential", "shuffle"):
        raise ValueError(f"block-synchronous sweeps visit the positions in order sequential|shuffle, got {order!r}")
    if layout not in bl.LAYOUTS:
        raise ValueError(f"block layout {layout!r}: expected one of {bl.LAYOUTS}")
    S, B, L = int(samples_num), int(batch_size), int(max_len)
    W = bl.resolve_width(int(width), L)
    serial_kw = dict(verbose=verbose, gamma=gamma, ctl_signal=ctl_signal, print_every=print_every, pos_template=pos_template,
                     sample_tau=sample_tau, sample_seed=sample_seed, sample0=sample0)
    eng = get_engine(model, clip, tokenizer)
    if W > 1 and gamma is not None:
        from . import control
        chosen = control.configure(eng, clip, tokenizer, pos_template=pos_template, ctl_signal=ctl_signal)
        if chosen == "exact":
            logger.info(f"block width {W}: the exact control scorer is called with one position per step; falling back to block "
                        "width 1 (CZC_CONTROL=table polishes blocks)")
            W = 1
    if W <= 1:
        return run_generation_samples(order, S, img_name, model, clip, tokenizer, image_instance, token_mask, prompt, logger, L,
                                      top_k, temperature, alpha, beta, max_iters, B, **serial_kw)
    seed_len = len(prompt.split()) + 1
    batch = ref_utils.get_init_text(tokenizer, prompt, L, B)
    clip.compute_image_representation_from_image_instance(image_instance)
    if getattr(eng, "_precision_logged", None) is None:
        scale = _logit_scale_of(clip)
        logger.info(f"engine precision: {PRECISION_NAMES.get(eng.precision, eng.precision)}"
                    + (f" (exp(logit_scale) = {math.exp(scale):.1f})" if scale is not None else ""))
        eng._precision_logged = True
    nb = bl.n_blocks(L, W)
    order_lists, per_sample = [], []
    for _ in range(S):
        if order == "shuffle":
            order_list, sweeps = bl.shuffle_sweeps(L, max_iters, random)     # gen_utils.py:110-111 (process-global stream)
            order_lists.append(order_list)
        else:
            sweeps = [bl.sequential_order(L, W, layout)] * max_iters
        per_sample.append(bl.tied_positions(sweeps, W)[0])
    said = (f"block width {W}, " + (f"layout {layout}, " if order == "sequential" else "consecutive blocks of the permutation, ")
            + f"{nb} steps per sweep instead of {L}")
    groups, cap, image_of_row = bl.tied_rows(S * B, W, image_of_caption=np.tile(np.arange(B, dtype=np.int32), S))
    rows_pos = bl.caption_positions([per_sample[c // B] for c in range(S * B)])
    hp = Engine.hyper(alpha, beta, temperature, gamma, ctl_signal == "negative", control="pos" if pos_template is not None else None)
    tau = float(sample_tau or 0.0)
    keys = [dw.image_key(n) for n in img_name]
    row_draws = None if not tau else [dw.make_draw(dw.row_seed(sample_seed, keys[c % B], sample0 + c // B, j), tau)
                                      for c in range(S * B) for j in range(W)]
    init_rows = np.repeat(np.asarray(batch[0], dtype=np.int32)[None, :], S * B * W, axis=0)

    def polish(eng):
        eng.set_token_mask(_mask_to_numpy(token_mask))
        eng.set_option("memo_rows", memo_rows_setting())
        if gamma is not None:
            from . import control
            chosen = control.configure(eng, clip, tokenizer, pos_template=pos_template, ctl_signal=ctl_signal)
            if chosen != getattr(eng, "_control_logged", None):
                logger.info(f"control scores: {chosen}")
                eng._control_logged = chosen
        runner = _group_for(eng, S * B * W)
        emb = None
        if runner is not eng:
            from clip.clip import ImageEmbeds
            emb = image_instance.embeds if isinstance(image_instance, ImageEmbeds) else clip.last_image_embeds()
            runner.set_image_embeds(emb)
        if eng.precision == native.PREC_REFINE:
            runner.refine_guard(reset=True)
        out = runner.generate_rows_tied(init_rows, None, seed_len, top_k, rows_pos, [hp] * (S * B * W), row_draws, groups,
                                        image_of_row=image_of_row, snapshot_every=nb)
        if runner is not eng:
            eng.set_image_embeds(emb)
        return out, runner

    ids, cos = _polish_guarded(polish, eng, model, clip, tokenizer, image_instance, logger)
    if rows_pos.shape[0]:   # the caller's mask as after the last position the serial loop would have visited (utils.py:53-59)
        last = order_lists[-1][-1] if order == "shuffle" else L - 1
        ref_utils.update_token_mask(tokenizer, token_mask, L, int(last))
    lead = np.arange(S * B) * W   # a group's rows hold one sentence and one cosine: its first row speaks for the caption
    out = []
    for s in range(S):
        rows = lead[s * B:(s + 1) * B]
        drew = dw.describe(row_draws[s * B * W:(s + 1) * B * W] if row_draws else None)
        logger.info((f"Order_list:{order_lists[s]}" if order == "shuffle" else f"Order:{order}") + f" ({said})" + drew)
        out.append(_bookkeeping(order, ids[:, rows], cos[:, rows], tokenizer, img_name, logger, B, verbose, print_every))
    return out


def caption_blocks(width: int, layout: str, samples_num: int, run_type: str, img_name, model, clip, tokenizer, image_instance,
                   token_mask, logger, *, prompt="", batch_size=1, max_len=15, top_k=100, temperature=1.0, max_iter=500, alpha=0.7,
                   beta=1, generate_order="sequential", gamma=5, ctl_type="sentiment", style_type="positive", pos_type=None,
                   sample_tau=0.0, sample_seed=0, sample0=0):
    """`--block_width` of the two CLIs: what caption_samples returns, polished in block-synchronous sweeps by one
    run_generation_blocks call.  The visiting order is sequential or shuffle (ValueError otherwise)."""
    start_time = time.time()
    kw = dict(verbose=True)
    order, max_iters = caption_order(run_type, generate_order, ctl_type, max_iter, max_len)
    if order not in ("sequential", "shuffle"):
        raise ValueError(f"--block_width needs generate_order sequential|shuffle, got {generate_order!r}")
    if run_type != "caption" and ctl_type == "sentiment":
        kw.update(gamma=gamma, ctl_signal=style_type)
    elif run_type != "caption":
        logger.info(pos_type)
        kw.update(gamma=gamma, pos_template=pos_type)
    outs = run_generation_blocks(order, width, layout, samples_num, img_name, model, clip, tokenizer, image_instance, token_mask,
                                 prompt, logger, max_len, top_k, temperature, alpha, beta, max_iters, batch_size,
                                 sample_tau=sample_tau, sample_seed=sample_seed, sample0=sample0, **kw)
    logger.info("Finished %d samples in %.3fs" % (samples_num, time.time() - start_time))
    for sample_id, (generate_texts, _) in enumerate(outs):
        logger.info(f"Sample {sample0 + sample_id}: ")
        for i in range(batch_size):
            logger.info(f"The {i + 1}-th image: {img_name[i]}")
            logger.info(f"final caption: {generate_texts[-2][i]}")
            logger.info(f"best caption: {generate_texts[-1][i]}")
    return outs


def caption_lengths(lens: Sequence[int], samples_num: int, run_type: str, img_name, model, clip, tokenizer, image_instance, token_mask,
                    logger, *, prompt="", batch_size=1, top_k=100, temperature=1.0, max_iter=500, alpha=0.7, beta=1,
                    generate_order="sequential", gamma=5, ctl_type="sentiment", style_type="positive", pos_type=None,
                    sample_tau=0.0, sample_seed=0, sample0=0):
    """`--sentence_lens` of the two CLIs: what `samples_num` calls of generate_caption (run_type 'caption') or
    control_generate_caption at max_len = n return for every n of `lens`, from one run_generation_lengths call.  Returns, per
    length, the list of `samples_num` (generate_texts, clip_scores) pairs and logs every length's and sample's final and best
    captions as those functions do.  The visiting order is sequential or shuffle (a caption run's `random` and `span` orders
    have no per-length schedule: ValueError)."""
    start_time = time.time()
    kw = dict(verbose=True)
    lens = [int(n) for n in lens]
    if not lens:
        raise ValueError("caption_lengths: no sentence lengths given")
    order, max_iters = caption_order(run_type, generate_order, ctl_type, max_iter, max(lens))
    if order not in ("sequential", "shuffle"):
        raise ValueError(f"sentence lengths in one call need generate_order sequential|shuffle, got {generate_order!r}")
    if run_type != "caption" and ctl_type == "sentiment":
        kw.update(gamma=gamma, ctl_signal=style_type)
    elif run_type != "caption":
        logger.info(pos_type)
        kw.update(gamma=gamma, pos_template=pos_type)
    outs = run_generation_lengths(order, lens, samples_num, img_name, model, clip, tokenizer, image_instance, token_mask, prompt,
                                  logger, top_k, temperature, alpha, beta, max_iters, batch_size,
                                  sample_tau=sample_tau, sample_seed=sample_seed, sample0=sample0, **kw)
    logger.info("Finished %d lengths x %d samples in %.3fs" % (len(lens), samples_num, time.time() - start_time))
    for n, per_sample in zip(lens, outs):
        for sample_id, (generate_texts, _) in enumerate(per_sample):
            logger.info(f"Sentence length {n}, sample {sample_id}: ")
            for i in range(batch_size):
                logger.info(f"The {i + 1}-th image: {img_name[i]}")
                logger.info(f"final caption: {generate_texts[-2][i]}")
                logger.info(f"best caption: {generate_texts[-1][i]}")
    return outs


def _signal_kw(signal: str, gamma, pos_type) -> dict:
    """The gamma / ctl_signal / pos_template keywords of the run_generation call behind `signal`."""
    from . import signals as sg
    run_type, ctl_type, style = sg.signal_run(signal)
    if run_type == "caption":
        return {}
    if ctl_type == "sentiment":
        return dict(gamma=gamma, ctl_signal=style)
    return dict(gamma=gamma, pos_template=pos_type)


def run_generation_signals(signals: Sequence[str], lens: Sequence[int], samples_num: int, generate_order: str, img_name, model, clip,
                           tokenizer, image_instance, token_mask, prompt, logger, top_k, temperature, alpha, beta, max_iter,
                           batch_size, verbose=True, gamma=5, pos_template=None, sample_tau: float = 0.0, sample_seed: int = 0,
                           sample0: int = 0):
    """The loop over control signals around the loops over lengths and samples (one CLI run per --run_type / --control_type /
    --sentiment_type) as ONE engine call: every signal x length x sample of a batch of `batch_size` images is a row of
    czc_generate_rows_hp with its own czc_hyper (signals.expand / signals.batch_rows), at its own length and with the visiting
    order the serial loop -- signals outside, then lengths, then samples -- would have drawn for it.  The control tables (lexicon
    and POS tags) are configured once and the images encoded once.  Returns, per signal, what run_generation_lengths returns
    for it (per length a list of `samples_num` (gen_texts_list, clip_score_sequence) pairs) and logs every call's lines in the
    serial loop's order.  The reference's own sentence scorer (exact control mode) is configured for one signal: with it the
    signals run one call each, as the serial loop runs them, and the log says why.
    `sample_tau` > 0: every row draws its winner (czc_generate_rows_draw) under draws.row_seed(sample_seed, key of the image's
    name, sample0 + s, g * len(lens) + l)."""
    import utils as ref_utils
    from . import control, draws as dw, signals as sg
    signals = sg.parse_signals(signals)
    lens = [int(n) for n in lens]
    S, B, NL = int(samples_num), int(batch_size), len(lens)
    if "pos" in signals and pos_template is None:
        raise ValueError("run_generation_signals: the pos signal needs a POS template")
    eng = get_engine(model, clip, tokenizer)
    # which control scores would each controlled signal get (control.configure's rule)?  The host scorer serves one signal.
    mode = control.control_mode()
    kinds = sorted({sg.signal_run(s)[1] == "pos" for s in signals if s != "caption"})
    exact = False
    for is_pos in kinds:
        explicit = (getattr(clip, "pos_tags", None) is not None) if is_pos else (
            getattr(clip, "lexicon_pos", None) is not None or getattr(clip, "lexicon", None) is not None)
        exact = exact or (not (explicit and mode != "exact") and mode in ("exact", "auto"))
    if exact:
        if not getattr(eng, "_one_by_one_signals_logged", False):
            logger.info("control signals: the exact control scorer is configured for one signal; running the "
                        f"{len(signals)} signals one call at a time (CZC_CONTROL=table batches them)")
            eng._one_by_one_signals_logged = True
        out = []
        for g, sig in enumerate(signals):
            order, max_iters = sg.signal_order(sig, generate_order, max_iter, max(lens))
            out.append(run_generation_lengths(order, lens, S, img_name, model, clip, tokenizer, image_instance, token_mask, prompt, logger,
                                              top_k, temperature, alpha, beta, max_iters, B, verbose=verbose, sample_tau=sample_tau,
                                              sample_seed=sample_seed, sample0=sample0, column0=g * NL,
                                              **_signal_kw(sig, gamma, pos_template)))
        return out
    seed_len = len(prompt.split()) + 1
    rows = sg.expand(signals, lens, S, generate_order, max_iter, alpha=alpha, beta=beta, temperature=temperature, gamma=gamma)
    clip.compute_image_representation_from_image_instance(image_instance)   # once per image, whatever the signals
    if getattr(eng, "_precision_logged", None) is None:
        scale = _logit_scale_of(clip)
        logger.info(f"engine precision: {PRECISION_NAMES.get(eng.precision, eng.precision)}"
                    + (f" (exp(logit_scale) = {math.exp(scale):.1f})" if scale is not None else ""))
        eng._precision_logged = True
    init_rows, row_lens, rows_pos, hypers, image_of_row = sg.batch_rows(rows, tokenizer, prompt, B)
    row_draws = dw.sample_rows(sample_seed, [dw.image_key(n) for n in img_name], S, float(sample_tau or 0.0),
                               columns=len(signals) * NL, sample0=sample0)

    def polish(eng):
        eng.set_token_mask(_mask_to_numpy(token_mask))
        eng.set_option("memo_rows", memo_rows_setting())  # per-row step memo of the rows call (CZC_MEMO_ROWS)
        for is_pos in kinds:   # both tables, once: a row reads the one its control names
            chosen = control.configure(eng, clip, tokenizer, pos_template=pos_template if is_pos else None)
            if chosen != getattr(eng, "_control_logged", None):
                logger.info(f"control scores: {chosen}")
                eng._control_logged = chosen
        runner = _group_for(eng, len(hypers))
        emb = None
        if runner is not eng:
            from clip.clip import ImageEmbeds
            emb = image_instance.embeds if isinstance(image_instance, ImageEmbeds) else clip.last_image_embeds()
            runner.set_image_embeds(emb)
        if eng.precision == native.PREC_REFINE:
            runner.refine_guard(reset=True)
        if row_draws is not None:
            res = runner.generate_rows_draw(init_rows, row_lens, seed_len, top_k, rows_pos, hypers, row_draws, image_of_row=image_of_row,
                                            n_mask=rows.n_mask, snapshot_every=rows.every)
        else:
            res = runner.generate_rows_hp(init_rows, row_lens, seed_len, top_k, rows_pos, hypers, image_of_row=image_of_row,
                                          n_mask=rows.n_mask, snapshot_every=rows.every)
        if runner is not eng:
            eng.set_image_embeds(emb)
        return res, runner

    ids, cos = _polish_guarded(polish, eng, model, clip, tokenizer, image_instance, logger)
    if rows.positions.shape[0]:   # the caller's mask as after the LAST call's last position: the last sample at the last length
        n = rows.col_lens[-1]
        ref_utils.update_token_mask(tokenizer, token_mask, n, int(rows.positions[(rows.sweeps - 1) * rows.every + n - 1, -1]))
    out = []
    for g, sig in enumerate(signals):
        if sig == "pos":
            logger.info(pos_template)
        per_len = []
        for l, n in enumerate(lens):
            per_sample = []
            for s in range(S):
                c = rows.column(g, l, s)
                said = dw.describe(row_draws[c * B:(c + 1) * B] if row_draws else None)
                if rows.orders[g] == "shuffle":
                    logger.info(f"Order_list:{[int(p) for p in rows.positions[:n, c]]}" + said)
                elif said:
                    logger.info(f"Order:{rows.orders[g]}" + said)
                per_sample.append(_bookkeeping(rows.orders[g], ids[:, c * B:(c + 1) * B, :seed_len + n + 1], cos[:, c * B:(c + 1) * B],
                                               tokenizer, img_name, logger, B, verbose, None))
            per_len.append(per_sample)
        out.append(per_len)
    return out


def caption_signals(signals: Sequence[str], lens: Sequence[int], samples_num: int, img_name, model, clip, tokenizer, image_instance,
                    token_mask, logger, *, prompt="", batch_size=1, top_k=100, temperature=1.0, max_iter=500, alpha=0.7, beta=1,
                    generate_order="sequential", gamma=5, pos_type=None, sample_tau=0.0, sample_seed=0, sample0=0):
    """`--signals` of the two CLIs: what `samples_num` calls of generate_caption (signal `caption`) or control_generate_caption
    (`positive`, `negative`: ctl_type sentiment; `pos`: ctl_type pos) at max_len = n return for every signal and every n of
    `lens`, from one run_generation_signals call.  Returns, per signal, per length, the list of `samples_num` (generate_texts,
    clip_scores) pairs and logs every signal's, length's and sample's final and best captions as those functions do."""
    from . import signals as sg
    start_time = time.time()
    signals = sg.parse_signals(signals)
    lens = [int(n) for n in lens]
    if not lens:
        raise ValueError("caption_signals: no sentence length given")
    outs = run_generation_signals(signals, lens, samples_num, generate_order, img_name, model, clip, tokenizer, image_instance,
                                  token_mask, prompt, logger, top_k, temperature, alpha, beta, max_iter, batch_size, gamma=gamma,
                                  pos_template=pos_type, sample_tau=sample_tau, sample_seed=sample_seed, sample0=sample0)
    logger.info("Finished %d signals x %d lengths x %d samples in %.3fs" % (len(signals), len(lens), samples_num, time.time() - start_time))
    for sig, per_len in zip(signals, outs):
        for n, per_sample in zip(lens, per_len):
            for sample_id, (generate_texts, _) in enumerate(per_sample):
                logger.info(f"Signal {sig}, sentence length {n}, sample {sample_id}: ")
                for i in range(batch_size):
                    logger.info(f"The {i + 1}-th image: {img_name[i]}")
                    logger.info(f"final caption: {generate_texts[-2][i]}")
                    logger.info(f"best caption: {generate_texts[-1][i]}")
    return outs


# ---- caption retrieval (conzic_amd/retrieval.py; czc_index_search) -------------------------------------------------------------
def retrieve_captions(index, img_name, model, clip, tokenizer, image_instance, logger, k: int = 1):
    """The reference's retrieval baseline (clip/clipretrieval.py `search_text`) for a batch and any k: per image of
    `image_instance` the k captions of `index` (retrieval.TextIndex) nearest to it, as (caption, cosine, id), best first.  The
    images are encoded once and scored against the engine's resident index in one czc_index_search call."""
    if model is not None:
        get_engine(model, clip, tokenizer)   # the index lives on the engine the generation calls use
    hits = index.search(clip, image_instance, k)
    for b, per_image in enumerate(hits):
        for j, (caption, cosine, row) in enumerate(per_image):
            logger.info(f"The {b + 1}-th image: {img_name[b]}, retrieved {j + 1}/{len(per_image)} (row {row}), "
                        f"clip score {cosine:.3f}: {caption}")
    return hits


def draft_skip_reason(tokenizer, prompt: str, caption: str) -> Optional[str]:
    """Why `caption` cannot be a draft row of run_infill, or None: infill.parse_template must give it at least one token behind the
    prompt and at most CZC_MAX_BERT_LEN tokens with [CLS], the prompt and [SEP]."""
    from . import infill
    try:
        ids, _, L, _ = infill.parse_template(tokenizer, prompt, caption)
    except ValueError as exc:
        return str(exc)
    if L < 1:
        return "empty after tokenising"
    if int(ids.size) > native.MAX_BERT_LEN:
        return f"{int(ids.size)} tokens with the prompt, more than the {native.MAX_BERT_LEN} a row holds"
    return None


def retrieve_then_polish(index, img_name, model, clip, tokenizer, image_instance, token_mask, prompt, logger, *, k: int = 1,
                         **run_infill_kwargs):
    """Start the Gibbs polish from the nearest known captions instead of from [MASK]s: the k retrieved captions of every image
    are the drafts of ONE run_infill(..., positions="all", image_of_caption=...) call.  A caption that cannot be a draft
    (draft_skip_reason) is skipped and logged.  Returns one dict per image: "retrieved": [(caption, cosine, id), ...] as
    retrieve_captions gives them, "drafts": the positions in that list of the captions that were polished, "polished": run_infill's
    (gen_texts_list, clip_score_sequence) pair of each of those, in the same order."""
    for fixed in ("positions", "image_of_caption"):
        if fixed in run_infill_kwargs:
            raise TypeError(f"retrieve_then_polish sets run_infill's {fixed} itself")
    hits = retrieve_captions(index, img_name, model, clip, tokenizer, image_instance, logger, k=k)
    out = [dict(retrieved=per_image, drafts=[], polished=[]) for per_image in hits]
    drafts, image_of_caption = [], []
    for b, per_image in enumerate(hits):
        for j, (caption, _, row) in enumerate(per_image):
            why = draft_skip_reason(tokenizer, prompt, caption)
            if why is not None:
                logger.info(f"The {b + 1}-th image: {img_name[b]}, retrieved caption {j + 1} (row {row}) is not polished: {why}")
                continue
            out[b]["drafts"].append(j)
            drafts.append(caption)
            image_of_caption.append(b)
    if drafts:
        from clip.clip import ImageEmbeds
        polished = run_infill(drafts, img_name, model, clip, tokenizer, ImageEmbeds(clip.last_image_embeds()), token_mask, prompt,
                              logger, positions="all", image_of_caption=image_of_caption, **run_infill_kwargs)
        for b, res in zip(image_of_caption, polished):
            out[b]["polished"].append(res)
    return out


def retrieve_cli(index, polish: bool, img_name, model, clip, tokenizer, image_instance, token_mask, logger, *, k=1, prompt="",
                 top_k=100, temperature=1.0, max_iter=10, alpha=0.7, beta=1, generate_order="sequential"):
    """`--run_type retrieve [--polish]` of the two CLIs; returns what retrieve_then_polish returns (without --polish: nothing
    polished), logging every polished caption's final and best text as infill_captions does."""
    start_time = time.time()
    if not polish:
        out = [dict(retrieved=h, drafts=[], polished=[])
               for h in retrieve_captions(index, img_name, model, clip, tokenizer, image_instance, logger, k=k)]
    else:
        out = retrieve_then_polish(index, img_name, model, clip, tokenizer, image_instance, token_mask, prompt, logger, k=k,
                                   order="sequential" if generate_order == "sequential" else "shuffle", max_iters=max_iter,
                                   top_k=top_k, temperature=temperature, alpha=alpha, beta=beta)
        for b, res in enumerate(out):
            for j, (generate_texts, _) in zip(res["drafts"], res["polished"]):
                logger.info(f"The {b + 1}-th image: {img_name[b]}, draft: {res['retrieved'][j][0]}")
                logger.info(f"final caption: {generate_texts[-2][0] if len(generate_texts) > 1 else 'None'}")
                logger.info(f"best caption: {generate_texts[-1][0]}")
    logger.info("Finished in %.3fs" % (time.time() - start_time))
    return out
