"""Harness in the role of the reference's run.py (directory of images, batches, JSON results):
same batching semantics -- `os.listdir` order, `batch_size`, `drop_last=True` (run.py:156-178) --
and the same on-disk layout (run.py:194-222):

    results/<run>_<order>_len<L>_topk<K>_alpha<a>_beta<b>_gamma<g>_lmTemp<t>/sample_<n>/iter_<k>.json
    .../best_clipscore.json        each a {image_name: caption} dict

    python -m conzic_amd.run_cli --synthetic --caption_img_path <dir> --run_type caption --order shuffle
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from conzic_amd.demo_cli import get_args  # same options as demo.py/run.py (run.py:15-76)


def result_dir(args, run_type, sample_id):
    """run.py:196-197 / :210-211"""
    prefix = "caption" if args.run_type == "caption" else run_type
    return "results/%s_%s_len%d_topk%d_alpha%.3f_beta%.3f_gamma%.3f_lmTemp%.3f/sample_%d" % (
        prefix, args.order, args.sentence_len, args.candidate_k, args.alpha, args.beta, args.gamma,
        args.lm_temperature, sample_id)


def merge_results(all_results, gen_texts, names):
    """run.py:86-92: all_results[iter_id][image_name] = caption (last entry = best-by-CLIP caption)."""
    for iter_id, texts in enumerate(gen_texts):
        if all_results[iter_id] is None:
            all_results[iter_id] = {}
        for name, text in zip(names, texts):
            all_results[iter_id][name] = text
    return all_results


def write_results(save_dir, all_results):
    """run.py:198-207"""
    os.makedirs(save_dir, exist_ok=True)
    for iter_id, res in enumerate(all_results):
        fn = "best_clipscore.json" if iter_id == len(all_results) - 1 else f"iter_{iter_id}.json"
        with open(os.path.join(save_dir, fn), "w") as f:
            json.dump(res, f)


def batches(names, batch_size):
    """DataLoader(shuffle=False, drop_last=True) over os.listdir order (run.py:158-178)."""
    for s in range(0, len(names) - batch_size + 1, batch_size):
        yield names[s:s + batch_size]


def region_rows(name_batch, region_map):
    """--regions_file: the rows of a batch of pictures -> (names, group_of_image).  A picture with an entry gives one row per box,
    named regions.region_name(name, box); a picture without gives one row under its own name.  group_of_image[i] = the position
    in `name_batch` of the picture row i was cut from.  Without a map: the batch itself."""
    if not region_map:
        return list(name_batch), list(range(len(name_batch)))
    from conzic_amd.regions import region_name
    names, groups = [], []
    for g, name in enumerate(name_batch):
        boxes = region_map.get(name)
        names.extend([name] if boxes is None else [region_name(name, b) for b in boxes])
        groups.extend([g] * (1 if boxes is None else len(boxes)))
    return names, groups


def load_batch(img_dir, name_batch, region_map):
    """The images of a batch as the encoder takes them: a picture with an entry in the map as clip.ImageRegions (all its boxes
    staged by one device call), the others whole, as without the map."""
    from PIL import Image
    from clip.clip import ImageRegions
    imgs = [Image.open(os.path.join(img_dir, n)).convert("RGB") for n in name_batch]
    if not region_map:
        return imgs
    return [ImageRegions(im, region_map[n]) if n in region_map else im for im, n in zip(imgs, name_batch)]


def region_rivals(args, clip, imgs, groups):
    """--distinct: the M nearest others of the batch, or under --regions_file the table scoped to the picture -- a region against
    the other regions of its picture (rivals.rival_table's group_of_image; a picture captioned whole is a group of one and gets
    no rivals)."""
    if not args.distinct:
        return None
    if args.regions_file is None:
        return args.distinct_rivals
    import numpy as np
    from clip.clip import ImageEmbeds
    from conzic_amd import rivals as rv
    emb = imgs.embeds if isinstance(imgs, ImageEmbeds) else np.asarray(clip.compute_image_representation_from_image_instance(imgs),
                                                                       dtype=np.float32)
    if len(groups) < 2:
        raise SystemExit("--distinct needs rival images: at least two rows in a batch")
    return rv.rival_table(emb, min(args.distinct_rivals, len(groups) - 1), group_of_image=groups)


def batched_samples(args, run_type, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask,
                    logger):
    """--batch_samples: every batch polishes its samples_num samples in one engine call (runtime.run_generation_samples).  The
    visiting orders of ALL (sample, batch) pairs are drawn first, in the sample loop's order, so every pair sees the order it
    sees without the flag (and every rank the same ones); the files are written sample for sample as without it."""
    from PIL import Image
    from conzic_amd.harness import sample_schedules
    from conzic_amd.runtime import caption_order, caption_samples
    from conzic_amd import vocab as vc
    vocab = vc.from_arguments(args, lm_tokenizer)   # --ban_words / --allow_words / --ban_per_sample: the same sets for every batch
    S, nb = args.samples_num, len(all_batches)
    order, max_iters = caption_order(args.run_type, args.order, args.control_type, args.num_iterations, args.sentence_len)
    positions, n_mask, every, order_lists = sample_schedules(order, args.sentence_len, max_iters, S * nb)
    results = [[None] * (args.num_iterations + 1) for _ in range(S)]
    for batch_idx, name_batch in enumerate(all_batches):
        if not (own_lo <= batch_idx < own_hi):
            continue
        logger.info(f"The {batch_idx + 1}-th batch:")
        cols = [s * nb + batch_idx for s in range(S)]   # the serial loop walks samples outside, batches inside
        sched = (positions[:, cols], n_mask, every, None if order_lists is None else [order_lists[c] for c in cols])
        imgs = load_batch(img_dir, name_batch, args.region_map)
        name_batch, groups = region_rows(name_batch, args.region_map)   # (--regions_file: one row per box)
        fluency = [] if args.fluency else False   # --fluency: this batch's records (runtime._fluency_after)
        outs = caption_samples(S, args.run_type, name_batch, lm_model, clip, lm_tokenizer, imgs, token_mask, logger,
                               prompt=args.prompt, batch_size=len(name_batch), max_len=args.sentence_len, top_k=args.candidate_k,
                               temperature=args.lm_temperature, max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta,
                               generate_order=args.order, gamma=args.gamma, ctl_type=args.control_type,
                               style_type=args.sentiment_type, pos_type=args.pos_type, schedules=sched,
                               sample_tau=args.sample_tau, sample_seed=args.seed,
                               rivals=region_rivals(args, clip, imgs, groups), delta=args.distinct, fluency=fluency,
                               vocab=vocab)
        if S > 1:
            from conzic_amd.diversity import log_distinct
            log_distinct(logger, name_batch, [[o[0][-2 if len(o[0]) > 1 else -1][i] for o in outs] for i in range(len(name_batch))])
        if args.pick_lambda is not None:
            from conzic_amd.runtime import log_picked
            log_picked(logger, name_batch, fluency, args.pick_lambda, lm_tokenizer)
        for s, (gen_texts, _) in enumerate(outs):
            results[s] = merge_results(results[s], gen_texts, name_batch)
    for sample_id in range(S):
        all_results = results[sample_id]
        if world > 1:
            import torch.distributed as tdist
            parts = [None] * world
            tdist.all_gather_object(parts, all_results)
            all_results = [None] * (args.num_iterations + 1)
            for part in parts:  # rank order == batch order
                for it, d in enumerate(part):
                    if d is not None:
                        all_results[it] = {**(all_results[it] or {}), **d}
        if rank == 0:
            write_results(result_dir(args, run_type, sample_id), all_results)


def lengths_batches(args, run_type, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask,
                    logger):
    """--sentence_lens: every batch polishes all lengths of a sample in one engine call (runtime.caption_lengths), or with
    --batch_samples all lengths of all its samples; the images are encoded once per batch.  The orders are drawn as that loop
    draws them -- samples outside and batches inside (with --batch_samples: batch by batch), lengths then samples inside a call --
    and a rank draws those of the batches it does not own as well.  The files are written per length and sample in the layout of
    a --sentence_len run at that length."""
    import copy
    from PIL import Image
    from clip.clip import ImageEmbeds
    from conzic_amd.runtime import advance_order_rng, caption_lengths, caption_order
    S, lens = args.samples_num, args.sentence_lens
    per_call = S if args.batch_samples else 1
    order, _ = caption_order(args.run_type, args.order, args.control_type, args.num_iterations, max(lens))
    results = [[[None] * (args.num_iterations + 1) for _ in range(S)] for _ in lens]
    embed_cache = {}
    for sample_id in ([None] if args.batch_samples else range(S)):
        if sample_id is not None:
            logger.info(f"Sample {sample_id + 1}: ")
        for batch_idx, name_batch in enumerate(all_batches):
            if not (own_lo <= batch_idx < own_hi):
                for n in lens:
                    for _ in range(per_call):
                        advance_order_rng(order, n, args.num_iterations)
                continue
            logger.info(f"The {batch_idx + 1}-th batch:")
            if batch_idx in embed_cache:
                imgs = ImageEmbeds(embed_cache[batch_idx])
            else:
                imgs = load_batch(img_dir, name_batch, args.region_map)
            name_batch, _ = region_rows(name_batch, args.region_map)   # (--regions_file: one row per box)
            outs = caption_lengths(lens, per_call, args.run_type, name_batch, lm_model, clip, lm_tokenizer, imgs, token_mask, logger,
                                   prompt=args.prompt, batch_size=len(name_batch), top_k=args.candidate_k,
                                   temperature=args.lm_temperature, max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta,
                                   generate_order=args.order, gamma=args.gamma, ctl_type=args.control_type,
                                   style_type=args.sentiment_type, pos_type=args.pos_type, sample_tau=args.sample_tau,
                                   sample_seed=args.seed, sample0=sample_id or 0)
            if batch_idx not in embed_cache:
                embed_cache[batch_idx] = clip.last_image_embeds()
            for l, per_sample in enumerate(outs):
                for s, (gen_texts, _) in enumerate(per_sample):
                    sid = s if sample_id is None else sample_id
                    results[l][sid] = merge_results(results[l][sid], gen_texts, name_batch)
    for l, n in enumerate(lens):
        at_len = copy.copy(args)
        at_len.sentence_len = n
        for sample_id in range(S):
            all_results = results[l][sample_id]
            if world > 1:
                import torch.distributed as tdist
                parts = [None] * world
                tdist.all_gather_object(parts, all_results)
                all_results = [None] * (args.num_iterations + 1)
                for part in parts:  # rank order == batch order
                    for it, d in enumerate(part):
                        if d is not None:
                            all_results[it] = {**(all_results[it] or {}), **d}
            if rank == 0:
                write_results(result_dir(at_len, run_type, sample_id), all_results)


def blocks_batches(args, run_type, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask,
                   logger):
    """--block_width: every batch polishes a sample's captions in block-synchronous sweeps, block_width tied rows per caption in
    one engine call (runtime.caption_blocks), or with --batch_samples those of all its samples; the images are encoded once per
    batch.  The orders are drawn as that loop draws them -- samples outside and batches inside (with --batch_samples: batch by
    batch) -- and a rank draws those of the batches it does not own as well.  The files are written sample for sample as
    without the flag."""
    from PIL import Image
    from clip.clip import ImageEmbeds
    from conzic_amd.runtime import advance_order_rng, caption_blocks, caption_order
    S = args.samples_num
    per_call = S if args.batch_samples else 1
    order, _ = caption_order(args.run_type, args.order, args.control_type, args.num_iterations, args.sentence_len)
    results = [[None] * (args.num_iterations + 1) for _ in range(S)]
    embed_cache = {}
    for sample_id in ([None] if args.batch_samples else range(S)):
        if sample_id is not None:
            logger.info(f"Sample {sample_id + 1}: ")
        for batch_idx, name_batch in enumerate(all_batches):
            if not (own_lo <= batch_idx < own_hi):
                for _ in range(per_call):
                    advance_order_rng(order, args.sentence_len, args.num_iterations)
                continue
            logger.info(f"The {batch_idx + 1}-th batch:")
            if batch_idx in embed_cache:
                imgs = ImageEmbeds(embed_cache[batch_idx])
            else:
                imgs = load_batch(img_dir, name_batch, args.region_map)
            name_batch, _ = region_rows(name_batch, args.region_map)   # (--regions_file: one row per box)
            outs = caption_blocks(args.block_width, args.block_layout, per_call, args.run_type, name_batch, lm_model, clip,
                                  lm_tokenizer, imgs, token_mask, logger, prompt=args.prompt, batch_size=len(name_batch),
                                  max_len=args.sentence_len, top_k=args.candidate_k, temperature=args.lm_temperature,
                                  max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta, generate_order=args.order,
                                  gamma=args.gamma, ctl_type=args.control_type, style_type=args.sentiment_type,
                                  pos_type=args.pos_type, sample_tau=args.sample_tau, sample_seed=args.seed, sample0=sample_id or 0)
            if batch_idx not in embed_cache:
                embed_cache[batch_idx] = clip.last_image_embeds()
            for s_, (gen_texts, _) in enumerate(outs):
                sid = s_ if sample_id is None else sample_id
                results[sid] = merge_results(results[sid], gen_texts, name_batch)
    for sample_id in range(S):
        all_results = results[sample_id]
        if world > 1:
            import torch.distributed as tdist
            parts = [None] * world
            tdist.all_gather_object(parts, all_results)
            all_results = [None] * (args.num_iterations + 1)
            for part in parts:  # rank order == batch order
                for it, d in enumerate(part):
                    if d is not None:
                        all_results[it] = {**(all_results[it] or {}), **d}
        if rank == 0:
            write_results(result_dir(args, run_type, sample_id), all_results)


def signals_batches(args, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask, logger):
    """--signals: every batch polishes all control signals (and with --sentence_lens all lengths) of a sample in one engine call
    (runtime.caption_signals), or with --batch_samples those of all its samples; the images are encoded once per batch.  The
    orders are drawn as that loop draws them -- samples outside and batches inside (with --batch_samples: batch by batch), then
    signals, lengths and samples inside a call -- and a rank draws those of the batches it does not own as well.  The files are
    written per signal, length and sample in the layout of a run of that signal at that length; the POS signal's directories
    start with `pos` (a --control_type pos run names its own after --sentiment_type, which a positive run here already uses)."""
    import copy
    from PIL import Image
    from clip.clip import ImageEmbeds
    from conzic_amd import signals as sg
    from conzic_amd.runtime import advance_order_rng, caption_signals
    S, sigs = args.samples_num, args.signals
    lens = args.sentence_lens or [args.sentence_len]
    per_call = S if args.batch_samples else 1
    orders = [sg.signal_order(g, args.order, args.num_iterations, max(lens))[0] for g in sigs]
    results = [[[[None] * (args.num_iterations + 1) for _ in range(S)] for _ in lens] for _ in sigs]
    embed_cache = {}
    for sample_id in ([None] if args.batch_samples else range(S)):
        if sample_id is not None:
            logger.info(f"Sample {sample_id + 1}: ")
        for batch_idx, name_batch in enumerate(all_batches):
            if not (own_lo <= batch_idx < own_hi):
                for order in orders:
                    for n in lens:
                        for _ in range(per_call):
                            advance_order_rng(order, n, args.num_iterations)
                continue
            logger.info(f"The {batch_idx + 1}-th batch:")
            if batch_idx in embed_cache:
                imgs = ImageEmbeds(embed_cache[batch_idx])
            else:
                imgs = load_batch(img_dir, name_batch, args.region_map)
            name_batch, _ = region_rows(name_batch, args.region_map)   # (--regions_file: one row per box)
            outs = caption_signals(sigs, lens, per_call, name_batch, lm_model, clip, lm_tokenizer, imgs, token_mask, logger,
                                   prompt=args.prompt, batch_size=len(name_batch), top_k=args.candidate_k,
                                   temperature=args.lm_temperature, max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta,
                                   generate_order=args.order, gamma=args.gamma, pos_type=args.pos_type, sample_tau=args.sample_tau,
                                   sample_seed=args.seed, sample0=sample_id or 0)
            if batch_idx not in embed_cache:
                embed_cache[batch_idx] = clip.last_image_embeds()
            for g, per_len in enumerate(outs):
                for l, per_sample in enumerate(per_len):
                    for s, (gen_texts, _) in enumerate(per_sample):
                        sid = s if sample_id is None else sample_id
                        results[g][l][sid] = merge_results(results[g][l][sid], gen_texts, name_batch)
    for g, sig in enumerate(sigs):
        for l, n in enumerate(lens):
            at = copy.copy(args)
            at.sentence_len = n
            at.run_type = "caption" if sig == "caption" else "controllable"
            for sample_id in range(S):
                all_results = results[g][l][sample_id]
                if world > 1:
                    import torch.distributed as tdist
                    parts = [None] * world
                    tdist.all_gather_object(parts, all_results)
                    all_results = [None] * (args.num_iterations + 1)
                    for part in parts:  # rank order == batch order
                        for it, d in enumerate(part):
                            if d is not None:
                                all_results[it] = {**(all_results[it] or {}), **d}
                if rank == 0:
                    write_results(result_dir(at, sig, sample_id), all_results)


def infill_batches(args, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask, logger):
    """--run_type infill: every --caption template is infilled for every image of a batch, all of them rows of one engine
    call (runtime.run_infill); the images are encoded once per batch.  One pass (sample_0): iter_<k>.json holds the
    captions after sweep k, keyed by image name (`name#c` for template c when there are several)."""
    from PIL import Image
    from conzic_amd.runtime import infill_captions
    C = len(args.caption)
    all_results = [None] * (args.num_iterations + 1)
    for batch_idx, name_batch in enumerate(all_batches):
        if not (own_lo <= batch_idx < own_hi):
            continue
        logger.info(f"The {batch_idx + 1}-th batch:")
        imgs = [Image.open(os.path.join(img_dir, n)).convert("RGB") for n in name_batch]
        caps = [c for _ in name_batch for c in args.caption]
        image_of_caption = [b for b in range(len(name_batch)) for _ in range(C)]
        outs = infill_captions(caps, name_batch, lm_model, clip, lm_tokenizer, imgs, token_mask, logger, prompt=args.prompt,
                               top_k=args.candidate_k, temperature=args.lm_temperature, max_iter=args.num_iterations,
                               alpha=args.alpha, beta=args.beta, generate_order=args.order, positions=args.infill_positions,
                               image_of_caption=image_of_caption, sample_tau=args.sample_tau, sample_seed=args.seed)
        for i, (gen_texts, _) in enumerate(outs):
            key = name_batch[i // C] if C == 1 else f"{name_batch[i // C]}#{i % C}"
            # (a batch whose captions have no blank at all returns no snapshots: its files repeat the best entry)
            texts = gen_texts[:-1] + [gen_texts[-2] if len(gen_texts) > 1 else gen_texts[-1]] * (args.num_iterations + 1 - len(gen_texts)) \
                + gen_texts[-1:]
            all_results = merge_results(all_results, texts, [key])
    if world > 1:
        import torch.distributed as tdist
        parts = [None] * world
        tdist.all_gather_object(parts, all_results)
        all_results = [None] * (args.num_iterations + 1)
        for part in parts:  # rank order == batch order
            for it, d in enumerate(part):
                if d is not None:
                    all_results[it] = {**(all_results[it] or {}), **d}
    if rank == 0:
        write_results(result_dir(args, "infill", 0), all_results)


def retrieve_batches(args, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask, logger):
    """--run_type retrieve: the --retrieve_k nearest index captions of every image (runtime.retrieve_captions), with --polish as
    the drafts of one polishing call per batch (runtime.retrieve_then_polish).  One pass (sample_0), keyed by image name (`name#j`
    for the j-th nearest when --retrieve_k > 1): without --polish best_clipscore.json holds the retrieved captions; with it
    iter_0.json holds them, iter_<s>.json the captions after sweep s and best_clipscore.json the best-by-CLIP ones (a caption that
    could not be a draft keeps its retrieved text throughout)."""
    from PIL import Image
    from conzic_amd.retrieval import index_from_args
    from conzic_amd.runtime import retrieve_cli
    index = index_from_args(args, clip, logger)
    K = args.retrieve_k
    n_files = args.num_iterations + 2 if args.polish else 1
    all_results = [None] * n_files
    for batch_idx, name_batch in enumerate(all_batches):
        if not (own_lo <= batch_idx < own_hi):
            continue
        logger.info(f"The {batch_idx + 1}-th batch:")
        imgs = [Image.open(os.path.join(img_dir, n)).convert("RGB") for n in name_batch]
        out = retrieve_cli(index, args.polish, name_batch, lm_model, clip, lm_tokenizer, imgs, token_mask, logger, k=K,
                           prompt=args.prompt, top_k=args.candidate_k, temperature=args.lm_temperature,
                           max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta, generate_order=args.order)
        for b, res in enumerate(out):
            polished = dict(zip(res["drafts"], res["polished"]))
            for j, (caption, _, _) in enumerate(res["retrieved"]):
                key = name_batch[b] if K == 1 else f"{name_batch[b]}#{j}"
                texts = [caption] * n_files
                if j in polished:
                    gen_texts = [t[0] for t in polished[j][0]]
                    sweeps = gen_texts[:-1] + [gen_texts[-2] if len(gen_texts) > 1 else caption] * (args.num_iterations + 1 - len(gen_texts))
                    texts = [caption] + sweeps + gen_texts[-1:]
                all_results = merge_results(all_results, [[t] for t in texts], [key])
    if world > 1:
        import torch.distributed as tdist
        parts = [None] * world
        tdist.all_gather_object(parts, all_results)
        all_results = [None] * n_files
        for part in parts:  # rank order == batch order
            for it, d in enumerate(part):
                if d is not None:
                    all_results[it] = {**(all_results[it] or {}), **d}
    if rank == 0:
        write_results(result_dir(args, "retrieve_polish" if args.polish else "retrieve", 0), all_results)


def main(argv=None):
    args = get_args(argv)
    if args.rival_images is not None:
        raise SystemExit("--rival_images belongs to conzic_amd.demo_cli; here the rivals of an image are its --distinct_rivals "
                         "nearest others in its batch")
    if args.regions is not None:
        raise SystemExit("--regions / --region_grid belong to conzic_amd.demo_cli; here: --regions_file FILE.json")
    args.region_map = None
    if args.regions_file is not None:
        from conzic_amd.regions import load_regions_file
        try:
            args.region_map = load_regions_file(args.regions_file)
        except (OSError, ValueError) as exc:
            raise SystemExit(f"--regions_file: {exc}")
    if args.distinct and args.batch_size < 2 and not args.region_map:
        raise SystemExit("--distinct needs rival images: a --batch_size of at least two")
    import logging
    import numpy as np
    from PIL import Image
    import utils
    from clip.clip import CLIP
    from control_gen_utils import control_generate_caption
    from gen_utils import generate_caption
    from conzic_amd import synth
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab

    utils.set_seed(args.seed)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    logger = logging.getLogger("ConZIC")
    run_type = "caption" if args.run_type == "caption" else "infill" if args.run_type == "infill" else args.sentiment_type
    if args.synthetic:
        sv = synth.make_vocab_tiny() if args.tiny else synth.make_vocab()
        bcfg = synth.bert_tiny(len(sv.bert_tokens)) if args.tiny else synth.bert_base()
        ccfg = synth.clip_tiny(len(sv.clip_vocab)) if args.tiny else synth.clip_b32()
        lm_tokenizer, clip_tok = tokenizers_from_vocab(sv)
        lm_model = SyntheticLM(bcfg)
        clip = CLIP.from_state(ccfg, synth.make_clip_weights(ccfg, 12), clip_tok)
        from conzic_amd import control
        if control.import_nltk() is None:
            # no nltk: synthetic per-token control tables (with nltk the runtime builds the tables from it, as it does
            # for real checkpoints -- conzic_amd/control.py; --control_scores exact calls the reference's scorer per step)
            clip.lexicon = synth.make_lexicon(len(sv.bert_tokens))
            clip.pos_tags = synth.make_pos_tags(len(sv.bert_tokens))
        token_mask = synth.make_token_mask(sv)
    else:
        from transformers import AutoModelForMaskedLM, AutoTokenizer
        lm_model = AutoModelForMaskedLM.from_pretrained(args.lm_model).eval()
        lm_tokenizer = AutoTokenizer.from_pretrained(args.lm_model)
        clip = CLIP(args.match_model)
        with open(args.stop_words_path, 'r', encoding='utf-8') as f:
            stop_words = [w.rstrip('\n') for w in f.readlines()]
        token_mask = np.ones((1, lm_tokenizer.vocab_size), dtype=np.float32)
        for sid in lm_tokenizer.convert_tokens_to_ids(stop_words):
            token_mask[0, sid] = 0
    img_dir = args.caption_img_path
    names = os.listdir(img_dir)
    # One process per GPU (torchrun): batches are block-partitioned over the ranks (conzic_amd/dist.py); every rank
    # walks ALL (sample, batch) pairs in the reference's order and advances the order RNG for the batches it skips,
    # so an N-rank run produces the single-process run's captions batch for batch.  No collective while polishing;
    # one gather of the caption dicts at the end of each sample.
    from conzic_amd import dist as czd
    from conzic_amd.runtime import advance_order_rng
    from clip.clip import ImageEmbeds
    rank, world, local = czd.env_rank_world()
    if world > 1:
        import torch
        import torch.distributed as tdist
        if torch.cuda.is_available():
            torch.cuda.set_device(local % torch.cuda.device_count())
            # host resources of this rank: the CPUs of its GPU's NUMA node, torch threads and scorer workers to match
            logger.info(f"rank {rank}: host share {czd.pin_rank(local, device_index=local % torch.cuda.device_count())}")
        if not tdist.is_initialized():
            tdist.init_process_group(os.environ.get("CZC_DIST_BACKEND", "nccl"))
    all_batches = list(batches(names, args.batch_size))
    own_lo, own_hi = czd.shard_range(len(all_batches), rank, world)
    embed_cache = {}  # batch index -> image_embeds [B, proj]: the ViT runs once per image, not once per sample
    if args.run_type == "retrieve":
        retrieve_batches(args, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask, logger)
        return
    if args.run_type == "infill":
        infill_batches(args, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask, logger)
        return
    if args.signals:
        signals_batches(args, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask, logger)
        return
    if args.sentence_lens:
        lengths_batches(args, run_type, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask,
                        logger)
        return
    if args.block_width != 1:
        blocks_batches(args, run_type, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer, token_mask,
                       logger)
        return
    if args.batch_samples:
        batched_samples(args, run_type, all_batches, own_lo, own_hi, rank, world, img_dir, lm_model, clip, lm_tokenizer,
                        token_mask, logger)
        return
    from conzic_amd import vocab as vc
    vocab = vc.from_arguments(args, lm_tokenizer)   # --ban_words / --allow_words (serial loop: one set for every sample)
    finals = {}   # image name -> the final caption of every sample
    fluency = {}  # --fluency: batch index -> the records of its final captions, every sample's (runtime._fluency_after)
    for sample_id in range(args.samples_num):
        all_results = [None] * (args.num_iterations + 1)
        logger.info(f"Sample {sample_id + 1}: ")
        for batch_idx, name_batch in enumerate(all_batches):
            if not (own_lo <= batch_idx < own_hi):
                advance_order_rng(args.order, args.sentence_len, args.num_iterations)
                continue
            logger.info(f"The {batch_idx + 1}-th batch:")
            if batch_idx in embed_cache:
                imgs = ImageEmbeds(embed_cache[batch_idx])
            else:
                imgs = load_batch(img_dir, name_batch, args.region_map)
            name_batch, groups = region_rows(name_batch, args.region_map)   # (--regions_file: one row per box)
            kw = dict(prompt=args.prompt, batch_size=len(name_batch), max_len=args.sentence_len,
                      top_k=args.candidate_k, temperature=args.lm_temperature, max_iter=args.num_iterations,
                      alpha=args.alpha, beta=args.beta, generate_order=args.order)
            if args.fluency:
                kw["fluency"] = fluency.setdefault(batch_idx, [])
                n_rec = len(kw["fluency"])
            if args.sample_tau or args.distinct or vocab is not None:   # the sample loop under --sample_tau / --distinct / word lists: one rows call per sample
                from conzic_amd.runtime import caption_samples
                (gen_texts, _), = caption_samples(1, args.run_type, name_batch, lm_model, clip, lm_tokenizer, imgs, token_mask, logger,
                                                  gamma=args.gamma, ctl_type=args.control_type, style_type=args.sentiment_type,
                                                  pos_type=args.pos_type, sample_tau=args.sample_tau, sample_seed=args.seed,
                                                  sample0=sample_id, rivals=region_rivals(args, clip, imgs, groups),
                                                  delta=args.distinct, vocab=vocab, **kw)
            elif args.run_type == 'caption':
                gen_texts, _ = generate_caption(name_batch, lm_model, clip, lm_tokenizer, imgs, token_mask, logger, **kw)
            else:
                gen_texts, _ = control_generate_caption(name_batch, lm_model, clip, lm_tokenizer, imgs, token_mask,
                                                        logger, gamma=args.gamma, ctl_type=args.control_type,
                                                        style_type=args.sentiment_type, pos_type=args.pos_type, **kw)
            if batch_idx not in embed_cache:
                embed_cache[batch_idx] = clip.last_image_embeds()
            if args.fluency:
                for rec in kw["fluency"][n_rec:]:
                    rec["sample"] = sample_id
            all_results = merge_results(all_results, gen_texts, name_batch)
            for name, text in zip(name_batch, gen_texts[-2 if len(gen_texts) > 1 else -1]):
                finals.setdefault(name, []).append(text)
        if world > 1:
            import torch.distributed as tdist
            parts = [None] * world
            tdist.all_gather_object(parts, all_results)
            all_results = [None] * (args.num_iterations + 1)
            for part in parts:  # rank order == batch order
                for it, d in enumerate(part):
                    if d is not None:
                        all_results[it] = {**(all_results[it] or {}), **d}
        if rank == 0:
            write_results(result_dir(args, run_type, sample_id), all_results)
    if args.samples_num > 1:   # (every rank logs the images of its own batches)
        from conzic_amd.diversity import log_distinct
        log_distinct(logger, list(finals), list(finals.values()))
    if args.pick_lambda is not None:
        from conzic_amd.runtime import log_picked
        for batch_idx, recs in sorted(fluency.items()):
            log_picked(logger, region_rows(all_batches[batch_idx], args.region_map)[0], recs, args.pick_lambda, lm_tokenizer)


if __name__ == "__main__":
    main()
