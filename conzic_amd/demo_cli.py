"""Harness in the role of the reference's demo.py / run.py (the callers of the boundary):
same option names and defaults (demo.py:15-76), same sequence of calls (demo.py:105-153):
set_seed once -> load LM / tokenizer / CLIP -> build token_mask from stop words -> loop samples
calling generate_caption / control_generate_caption.

    python -m conzic_amd.demo_cli --synthetic --run_type caption --order sequential
    python -m conzic_amd.demo_cli --lm_model <dir> --match_model <dir> --caption_img_path img.jpg ...
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def get_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--device", type=str, default='cuda', choices=['cuda'])
    p.add_argument('--run_type', default='controllable', nargs='?', choices=['caption', 'controllable', 'infill', 'retrieve'])
    p.add_argument('--prompt', default='Image of a', type=str)
    p.add_argument('--order', default='shuffle', nargs='?', choices=['sequential', 'shuffle', 'span', 'random'])
    p.add_argument('--control_type', default='sentiment', nargs='?', choices=["sentiment", "pos"])
    # demo.py:40-45 declares this with type=list (unusable from a shell); here: a JSON list of tag lists
    p.add_argument('--pos_type', type=json.loads,
                   default=[['DET'], ['ADJ', 'NOUN'], ['NOUN'], ['VERB'], ['VERB'], ['ADV'], ['ADP'], ['DET', 'NOUN'],
                            ['NOUN'], ['NOUN', '.'], ['.', 'NOUN'], ['.', 'NOUN']],
                   help="predefined part-of-speech template (JSON)")
    p.add_argument('--sentiment_type', default="positive", nargs='?', choices=["positive", "negative"])
    p.add_argument('--samples_num', default=2, type=int)
    p.add_argument("--sentence_len", type=int, default=10)
    p.add_argument("--candidate_k", type=int, default=200)
    p.add_argument("--alpha", type=float, default=0.02)
    p.add_argument("--beta", type=float, default=2.0)
    p.add_argument("--gamma", type=float, default=5.0)
    p.add_argument("--lm_temperature", type=float, default=0.1)
    p.add_argument("--num_iterations", type=int, default=10)
    p.add_argument("--lm_model", type=str, default='bert-base-uncased')
    p.add_argument("--match_model", type=str, default='openai/clip-vit-base-patch32')
    p.add_argument("--caption_img_path", type=str, default=None)
    p.add_argument("--stop_words_path", type=str, default=None)
    p.add_argument("--synthetic", action="store_true", help="random-init weights + synthetic vocab/images (no checkpoints)")
    p.add_argument("--tiny", action="store_true", help="with --synthetic: tiny model dims")
    p.add_argument("--control_scores", default=None, choices=["auto", "table", "exact"],
                   help="controllable runs: the reference's own nltk sentence scorer called back once per step (exact; what "
                        "auto picks when nltk imports) or per-token tables built from nltk and evaluated inside the engine's "
                        "kernels (table: the throughput mode, context-free approximation); sets CZC_CONTROL")
    p.add_argument("--batch_samples", action="store_true",
                   help="polish the samples_num samples of a batch in ONE engine call (one row per image and sample, every "
                        "sample with the visiting order the sample loop would have drawn for it) instead of one call per sample")
    p.add_argument("--sample_tau", type=float, default=0.0, metavar="T",
                   help="draw every step's winner from softmax_K(fused score / T) instead of taking the argmax (0 = off, the "
                        "reference's rule); every (image, sample) draws under its own seed derived from --seed, so samples_num "
                        "samples differ under any --order and repeat from run to run; combines with --batch_samples, "
                        "--sentence_lens, --signals and --run_type infill")
    p.add_argument("--sentence_lens", type=lambda v: [int(n) for n in v.split(",") if n.strip()], default=None, metavar="L1,L2,...",
                   help="several sentence lengths of every image in ONE engine call, e.g. 6,8,10,12 (each row at its own length; "
                        "--order sequential or shuffle): one call per sample, or with --batch_samples one call of samples_num x "
                        "len(lens) rows per image; --sentence_len is ignored while this is set")
    p.add_argument("--signals", type=lambda v: [g.strip().lower() for g in v.split(",") if g.strip()], default=None,
                   metavar="caption,positive,negative[,pos]",
                   help="one image under several control signals in ONE engine call (one row per signal, each with its own "
                        "hyper-parameters and the visiting order its own run would draw); combines with --sentence_lens and "
                        "--batch_samples; --run_type / --control_type / --sentiment_type are ignored while this is set")
    p.add_argument("--block_width", type=int, default=1, metavar="W",
                   help="block-synchronous sweeps: W tied rows per caption polish W positions of it per step, each from the same "
                        "current sentence, and all winners are written back together -- ceil(sentence_len / W) serial steps per "
                        "sweep instead of sentence_len (1 = off, the serial sweep; 0 = sentence_len, all positions at once); "
                        "--order sequential or shuffle; combines with --batch_samples and --sample_tau")
    p.add_argument("--block_layout", default="interleaved", choices=["interleaved", "contiguous"],
                   help="--block_width under --order sequential: a block holds every nb-th position (interleaved: neighbouring "
                        "words never update together) or W neighbouring positions (contiguous)")
    p.add_argument("--caption", action="append", default=None, metavar="TEMPLATE",
                   help="--run_type infill (repeatable): a caption with blanks, e.g. \"a _ dog on a _\"; only the blanks are "
                        "polished (num_iterations sweeps, --order sequential or shuffle over each caption's blanks), the given "
                        "words stay as context; all captions, whatever their token lengths, go through one engine call")
    p.add_argument("--infill_positions", default="blanks", choices=["blanks", "all"],
                   help="--run_type infill: polish the blanks only, or every position of every caption (polishing a draft / "
                        "resuming an earlier result)")
    p.add_argument("--index_matrix_path", type=str, default=None,
                   help="--run_type retrieve: the text index, one row of space-separated floats per caption (or .npy), as the "
                        "reference's clip/build_text_index.py writes it; with --mapping_dict_path")
    p.add_argument("--mapping_dict_path", type=str, default=None,
                   help="--run_type retrieve: JSON {row number: caption} of --index_matrix_path")
    p.add_argument("--index_captions", type=str, default=None, metavar="FILE",
                   help="--run_type retrieve: build the index on the spot from FILE, one caption per line, instead of loading one")
    p.add_argument("--retrieve_k", type=int, default=1, help="--run_type retrieve: nearest captions per image (1..64)")
    p.add_argument("--polish", action="store_true",
                   help="--run_type retrieve: the retrieved captions are the drafts of a Gibbs polish of every position "
                        "(num_iterations sweeps in --order sequential or shuffle, --candidate_k, alpha / beta / temperature), all "
                        "of them rows of one engine call")
    p.add_argument("--distinct", type=float, default=0.0, metavar="DELTA",
                   help="discriminative captions: add DELTA x P(own image | candidate) -- the softmax over the image and its rival "
                        "images of exp(logit_scale) x cos(candidate, image), taken at the own image -- to every candidate's fused "
                        "score, so that the caption says what tells this image from its look-alikes (0 = off); combines with "
                        "--batch_samples, --sample_tau and --run_type controllable")
    p.add_argument("--distinct_rivals", type=int, default=4, metavar="M",
                   help="--distinct: the rivals of an image are its M nearest others (image-image cosine) in its batch (1..16)")
    p.add_argument("--rival_images", type=lambda v: [f.strip() for f in v.split(",") if f.strip()], default=None, metavar="a.jpg,b.jpg",
                   help="demo_cli with --distinct: images that are rivals only (not captioned); every captioned image is scored "
                        "against all of them instead of against its batch neighbours")
    p.add_argument("--fluency", action="store_true",
                   help="after the last sweep, log every final caption's BERT pseudo-log-likelihood (the sum over its words of "
                        "log p(word | caption with that word masked)), mean log p, pseudo-perplexity and the word BERT ranks "
                        "lowest; changes neither the captions nor the files; combines with --batch_samples, --sample_tau, "
                        "--distinct and --run_type controllable")
    p.add_argument("--pick_lambda", type=float, default=None, metavar="LAMBDA",
                   help="implies --fluency; needs --samples_num > 1: log, per image, the \"picked caption\": the sample whose final "
                        "caption has the largest cosine + LAMBDA x mean log p (the \"best caption\" lines stay as they are)")
    p.add_argument("--regions", type=str, default=None, metavar="\"x0,y0,x1,y1;...\"",
                   help="demo_cli: caption these boxes of the picture instead of the whole picture (PIL's crop convention: pixel "
                        "coordinates, x1 and y1 exclusive); all boxes are cropped, resized and staged on the device in one call and "
                        "are the images of the batch from then on, so every other flag applies to them; with --distinct each box "
                        "is described by what sets it apart from the other boxes")
    p.add_argument("--region_grid", type=str, default=None, metavar="RxC",
                   help="demo_cli: the R x C tiles of the picture as regions (before those of --regions)")
    p.add_argument("--region_full", action="store_true",
                   help="demo_cli: with --regions / --region_grid, the whole frame as the first region")
    p.add_argument("--regions_file", type=str, default=None, metavar="FILE.json",
                   help="run_cli: JSON {file name: [[x0,y0,x1,y1], ...]}; an image with an entry is captioned box by box (keys "
                        "name#x0,y0,x1,y1 in the output files), one without is captioned whole; with --distinct the rivals of a "
                        "region are the other regions of its picture")
    from conzic_amd import vocab as vc
    vc.add_arguments(p)
    a = p.parse_args(argv)
    vc.check_arguments(p, a)
    if a.regions is not None or a.region_grid is not None:
        from conzic_amd import regions as rg
        try:
            a.regions = rg.parse_boxes(a.regions) if a.regions is not None else []
            a.region_grid = rg.parse_grid(a.region_grid) if a.region_grid is not None else None
        except ValueError as exc:
            p.error(f"--regions / --region_grid: {exc}")
        if a.batch_size != 1:
            p.error("--regions / --region_grid cut ONE picture into the images of the batch: --batch_size 1")
        if a.regions_file is not None:
            p.error("--regions / --region_grid belong to conzic_amd.demo_cli, --regions_file to conzic_amd.run_cli")
    elif a.region_full:
        p.error("--region_full adds the whole frame to --regions / --region_grid")
    if a.regions is not None or a.regions_file is not None:
        flag = "--regions_file" if a.regions_file is not None else "--regions / --region_grid"
        if a.run_type in ("infill", "retrieve"):
            p.error(f"{flag} does not combine with --run_type {a.run_type} (the engine call stages regions for any caller; the "
                    "command-line plumbing does not yet)")
        if a.rival_images is not None:
            p.error(f"{flag} does not combine with --rival_images (the rivals of a region are the other regions of its picture)")
    if a.pick_lambda is not None:
        if not (a.pick_lambda == a.pick_lambda) or a.pick_lambda in (float("inf"), float("-inf")):
            p.error("--pick_lambda must be finite")
        if a.samples_num <= 1:
            p.error("--pick_lambda chooses among the samples of an image: it needs --samples_num > 1")
        a.fluency = True
    if a.fluency:
        if a.run_type in ("infill", "retrieve"):
            p.error(f"--fluency does not combine with --run_type {a.run_type} (the engine call scores rows of any length; the "
                    "command-line plumbing does not yet)")
        for flag, on in (("--sentence_lens", a.sentence_lens is not None), ("--signals", a.signals is not None),
                         ("--block_width", a.block_width != 1)):
            if on:
                p.error(f"--fluency does not combine with {flag} (the engine call scores rows of any length; the command-line "
                        "plumbing does not yet)")
    if not (a.distinct == a.distinct) or a.distinct in (float("inf"), float("-inf")):
        p.error("--distinct must be finite")
    if a.distinct:
        if not 1 <= a.distinct_rivals <= 16:
            p.error("--distinct_rivals must be between 1 and 16")
        if a.rival_images is not None and not 1 <= len(a.rival_images) <= 16:
            p.error("--rival_images takes between 1 and 16 files")
        if a.run_type in ("infill", "retrieve"):
            p.error(f"--distinct does not combine with --run_type {a.run_type} (the engine call supports rivals there; the "
                    "command-line plumbing does not yet)")
        for flag, on in (("--sentence_lens", a.sentence_lens is not None), ("--signals", a.signals is not None),
                         ("--block_width", a.block_width != 1)):
            if on:
                p.error(f"--distinct does not combine with {flag} (the engine call supports rivals there; the command-line "
                        "plumbing does not yet)")
    elif a.rival_images is not None:
        p.error("--rival_images belongs to --distinct")
    if not (a.sample_tau >= 0.0) or a.sample_tau == float("inf"):
        p.error("--sample_tau must be finite and >= 0")
    if a.sample_tau and a.run_type == "retrieve":
        p.error("--sample_tau does not apply to --run_type retrieve")
    if a.block_width < 0:
        p.error("--block_width must be >= 0 (0 = the sentence length, 1 = off)")
    if a.block_width != 1:
        if a.run_type in ("infill", "retrieve"):
            p.error(f"--block_width does not combine with --run_type {a.run_type} (block-synchronous sweeps polish whole captions "
                    "of one length from the prompt)")
        if a.sentence_lens is not None:
            p.error("--block_width does not combine with --sentence_lens")
        if a.signals is not None:
            p.error("--block_width does not combine with --signals")
        if a.run_type == "caption" and a.order not in ("sequential", "shuffle"):
            p.error("--block_width cuts a sweep's visiting order into blocks: --order sequential or shuffle")
    if a.run_type == "retrieve":
        from conzic_amd import native
        files = a.index_matrix_path is not None or a.mapping_dict_path is not None
        if files and a.index_captions is not None:
            p.error("--run_type retrieve takes --index_matrix_path with --mapping_dict_path, or --index_captions, not both")
        if files and (a.index_matrix_path is None or a.mapping_dict_path is None):
            p.error("--index_matrix_path and --mapping_dict_path go together")
        if not files and a.index_captions is None:
            p.error("--run_type retrieve needs --index_matrix_path with --mapping_dict_path, or --index_captions")
        if not 1 <= a.retrieve_k <= native.INDEX_MAX_K:
            p.error(f"--retrieve_k must be between 1 and {native.INDEX_MAX_K}")
        if a.polish and a.order not in ("sequential", "shuffle"):
            p.error("--run_type retrieve --polish visits the positions in --order sequential or shuffle")
        if a.sentence_lens is not None:
            p.error("--sentence_lens does not apply to --run_type retrieve (a retrieved caption has its own length)")
        if a.signals is not None:
            p.error("--signals does not apply to --run_type retrieve")
        if a.caption:
            p.error("--caption belongs to --run_type infill")
    elif a.polish or a.index_matrix_path or a.mapping_dict_path or a.index_captions:
        p.error("--index_matrix_path / --mapping_dict_path / --index_captions / --polish belong to --run_type retrieve")
    if a.run_type == "infill" and not a.caption:
        p.error("--run_type infill needs at least one --caption")
    if a.run_type == "infill" and a.order not in ("sequential", "shuffle"):
        p.error("--run_type infill visits the blanks in --order sequential or shuffle")
    if a.sentence_lens is not None:
        if a.run_type == "infill":
            p.error("--sentence_lens does not apply to --run_type infill (a template has its own length)")
        if not a.sentence_lens or min(a.sentence_lens) < 1:
            p.error("--sentence_lens needs a comma-separated list of lengths >= 1")
        if a.run_type == "caption" and a.order not in ("sequential", "shuffle"):
            p.error("--sentence_lens visits every row's positions in --order sequential or shuffle")
    if a.signals is not None:
        from conzic_amd import signals as sg
        if a.run_type == "infill":
            p.error("--signals does not apply to --run_type infill")
        try:
            a.signals = sg.parse_signals(a.signals)
        except ValueError as exc:
            p.error(f"--signals: {exc}")
        if a.order not in ("sequential", "shuffle"):
            p.error("--signals visits every row's positions in --order sequential or shuffle")
    if a.control_scores:
        os.environ["CZC_CONTROL"] = a.control_scores
    return a


def main(argv=None):
    args = get_args(argv)
    import utils
    from clip.clip import CLIP
    from control_gen_utils import control_generate_caption
    from gen_utils import generate_caption
    from conzic_amd import synth
    from conzic_amd.models import SyntheticLM
    from conzic_amd.text import tokenizers_from_vocab
    import logging

    utils.set_seed(args.seed)
    logger = logging.getLogger("ConZIC")
    logging.basicConfig(level=logging.INFO, format="%(message)s")
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
        from PIL import Image
        images = [Image.fromarray(u) for u in synth.make_images_u8(args.batch_size, ccfg.v_image)]
    else:
        from transformers import AutoModelForMaskedLM, AutoTokenizer
        lm_model = AutoModelForMaskedLM.from_pretrained(args.lm_model).eval()
        lm_tokenizer = AutoTokenizer.from_pretrained(args.lm_model)
        clip = CLIP(args.match_model)
        with open(args.stop_words_path, 'r', encoding='utf-8') as f:          # demo.py:135-143
            stop_words = [w.rstrip('\n') for w in f.readlines()]
        token_mask = np.ones((1, lm_tokenizer.vocab_size), dtype=np.float32)
        for sid in lm_tokenizer.convert_tokens_to_ids(stop_words):
            token_mask[0, sid] = 0
        from PIL import Image
        images = [Image.open(args.caption_img_path).convert("RGB")]
    image_instance = images if args.batch_size > 1 else images[0]
    img_name = [f"img{j}" for j in range(args.batch_size)]
    if args.regions_file is not None:
        raise SystemExit("--regions_file belongs to conzic_amd.run_cli; here: --regions \"x0,y0,x1,y1;...\" / --region_grid RxC")
    if args.regions is not None:
        # the boxes of the picture are the images of the batch from here on: one regions call stages them all
        from clip.clip import ImageRegions
        from conzic_amd import regions as rg
        width, height = images[0].size
        try:
            boxes = ([(0, 0, width, height)] if args.region_full else []) \
                + (rg.grid_boxes(width, height, *args.region_grid) if args.region_grid else []) + list(args.regions)
            boxes = rg.check_boxes(boxes, width, height, clip._image_size())
        except ValueError as exc:
            raise SystemExit(f"--regions / --region_grid: {exc}")
        image_instance = ImageRegions(images[0], boxes)
        img_name = [rg.region_name(img_name[0], b) for b in boxes]   # (logs and the seeds of --sample_tau name the box)
        args.batch_size = len(boxes)
    rivals = args.distinct_rivals if args.distinct else None
    if args.distinct and args.regions is not None and args.batch_size >= 2:
        # rivals scoped to the picture: a region against the nearest other regions of the same picture
        from conzic_amd import rivals as rv
        emb = np.asarray(clip.compute_image_representation_from_image_instance(image_instance), dtype=np.float32)
        rivals = rv.rival_table(emb, min(args.distinct_rivals, args.batch_size - 1), group_of_image=[0] * args.batch_size)
    if args.distinct and args.rival_images:
        # the rival images ride behind the captioned ones in the resident batch; every captioned image is scored against all of them
        B, E = args.batch_size, len(args.rival_images)
        image_instance = list(images) + [Image.open(f).convert("RGB") for f in args.rival_images]
        rivals = np.tile(np.arange(B, B + E, dtype=np.int32), (B, 1))
    elif args.distinct and args.batch_size < 2:
        raise SystemExit("--distinct needs rival images: --rival_images a.jpg,b.jpg, or a batch of at least two images")
    t0 = time.time()
    if args.run_type == "retrieve":
        from conzic_amd.retrieval import index_from_args
        from conzic_amd.runtime import retrieve_cli
        retrieve_cli(index_from_args(args, clip, logger), args.polish, img_name, lm_model, clip, lm_tokenizer, image_instance,
                     token_mask, logger, k=args.retrieve_k, prompt=args.prompt, top_k=args.candidate_k,
                     temperature=args.lm_temperature, max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta,
                     generate_order=args.order)
        logger.info("total %.2fs" % (time.time() - t0))
        return
    if args.run_type == "infill":
        # caption i describes image i (batch_size captions), or every caption the one image (batch_size 1)
        from conzic_amd.runtime import infill_captions
        infill_captions(args.caption, img_name, lm_model, clip, lm_tokenizer, image_instance, token_mask, logger, prompt=args.prompt,
                        top_k=args.candidate_k, temperature=args.lm_temperature, max_iter=args.num_iterations, alpha=args.alpha,
                        beta=args.beta, generate_order=args.order, positions=args.infill_positions,
                        sample_tau=args.sample_tau, sample_seed=args.seed)
        logger.info("total %.2fs" % (time.time() - t0))
        return
    if args.signals:
        # all signals (and lengths) of a sample (with --batch_samples: of all samples) are rows of one engine call
        from conzic_amd.runtime import caption_signals
        for sample_id in ([None] if args.batch_samples else range(args.samples_num)):
            if sample_id is not None:
                logger.info(f"Sample {sample_id}: ")
            caption_signals(args.signals, args.sentence_lens or [args.sentence_len], args.samples_num if args.batch_samples else 1,
                            img_name, lm_model, clip, lm_tokenizer, image_instance, token_mask, logger, prompt=args.prompt,
                            batch_size=args.batch_size, top_k=args.candidate_k, temperature=args.lm_temperature,
                            max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta, generate_order=args.order,
                            gamma=args.gamma, pos_type=args.pos_type, sample_tau=args.sample_tau, sample_seed=args.seed,
                            sample0=sample_id or 0)
        logger.info("total %.2fs" % (time.time() - t0))
        return
    if args.sentence_lens:
        # all lengths of a sample (with --batch_samples: of all samples) are rows of one engine call
        from conzic_amd.runtime import caption_lengths
        kw = dict(prompt=args.prompt, batch_size=args.batch_size, top_k=args.candidate_k, temperature=args.lm_temperature,
                  max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta, generate_order=args.order, gamma=args.gamma,
                  ctl_type=args.control_type, style_type=args.sentiment_type, pos_type=args.pos_type,
                  sample_tau=args.sample_tau, sample_seed=args.seed)
        for sample_id in ([None] if args.batch_samples else range(args.samples_num)):
            if sample_id is not None:
                logger.info(f"Sample {sample_id}: ")
            caption_lengths(args.sentence_lens, args.samples_num if args.batch_samples else 1, args.run_type, img_name, lm_model, clip,
                            lm_tokenizer, image_instance, token_mask, logger, sample0=sample_id or 0, **kw)
        logger.info("total %.2fs" % (time.time() - t0))
        return
    from conzic_amd.diversity import log_distinct
    finals = [[] for _ in img_name]   # per image: the final caption of every sample
    fluency = [] if args.fluency else False   # --fluency: the records of every final caption (runtime._fluency_after)

    def pick():
        if args.pick_lambda is not None:
            from conzic_amd.runtime import log_picked
            log_picked(logger, img_name, fluency, args.pick_lambda, lm_tokenizer)

    def keep(generate_texts):
        last = generate_texts[-2] if len(generate_texts) > 1 else generate_texts[-1]   # (no snapshot recorded: the best entry)
        for i in range(args.batch_size):
            finals[i].append(last[i])

    if args.block_width != 1:
        # block-synchronous sweeps: the block_width tied rows of every caption (with --batch_samples: of all samples) in one call
        from conzic_amd.runtime import caption_blocks
        kw = dict(prompt=args.prompt, batch_size=args.batch_size, max_len=args.sentence_len, top_k=args.candidate_k,
                  temperature=args.lm_temperature, max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta,
                  generate_order=args.order, gamma=args.gamma, ctl_type=args.control_type,
                  style_type=args.sentiment_type, pos_type=args.pos_type, sample_tau=args.sample_tau, sample_seed=args.seed)
        for sample_id in ([None] if args.batch_samples else range(args.samples_num)):
            outs = caption_blocks(args.block_width, args.block_layout, args.samples_num if sample_id is None else 1, args.run_type,
                                  img_name, lm_model, clip, lm_tokenizer, image_instance, token_mask, logger,
                                  sample0=sample_id or 0, **kw)
            for generate_texts, _ in outs:
                keep(generate_texts)
        if args.samples_num > 1:
            log_distinct(logger, img_name, finals)
        logger.info("total %.2fs" % (time.time() - t0))
        return finals
    from conzic_amd import vocab as vc
    if args.batch_samples or args.sample_tau or args.distinct or vc.wanted(args):
        # one engine call for all samples, or -- the serial loop under --sample_tau / --distinct / the word lists -- one per sample
        # with that sample's seeds
        from conzic_amd.runtime import caption_samples
        kw = dict(prompt=args.prompt, batch_size=args.batch_size, max_len=args.sentence_len, top_k=args.candidate_k,
                  temperature=args.lm_temperature, max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta,
                  generate_order=args.order, gamma=args.gamma, ctl_type=args.control_type,
                  style_type=args.sentiment_type, pos_type=args.pos_type, sample_tau=args.sample_tau, sample_seed=args.seed,
                  rivals=rivals, delta=args.distinct, fluency=fluency, vocab=vc.from_arguments(args, lm_tokenizer))
        for sample_id in ([None] if args.batch_samples else range(args.samples_num)):
            outs = caption_samples(args.samples_num if sample_id is None else 1, args.run_type, img_name, lm_model, clip, lm_tokenizer,
                                   image_instance, token_mask, logger, sample0=sample_id or 0, **kw)
            for generate_texts, _ in outs:
                keep(generate_texts)
        if args.samples_num > 1:
            log_distinct(logger, img_name, finals)
        pick()
        logger.info("total %.2fs" % (time.time() - t0))
        return finals
    for sample_id in range(args.samples_num):                                   # demo.py:83 (no reseeding)
        logger.info(f"Sample {sample_id}: ")
        kw = dict(prompt=args.prompt, batch_size=args.batch_size, max_len=args.sentence_len, top_k=args.candidate_k,
                  temperature=args.lm_temperature, max_iter=args.num_iterations, alpha=args.alpha, beta=args.beta,
                  generate_order=args.order)
        n_rec = len(fluency) if args.fluency else 0
        if args.fluency:
            kw["fluency"] = fluency
        if args.run_type == 'caption':
            generate_texts, _ = generate_caption(img_name, lm_model, clip, lm_tokenizer, image_instance, token_mask, logger, **kw)
        else:
            generate_texts, _ = control_generate_caption(img_name, lm_model, clip, lm_tokenizer, image_instance, token_mask, logger,
                                                         gamma=args.gamma, ctl_type=args.control_type, style_type=args.sentiment_type,
                                                         pos_type=args.pos_type, **kw)
        keep(generate_texts)
        for rec in (fluency[n_rec:] if args.fluency else ()):
            rec["sample"] = sample_id   # (run_generation does not know which sample of the loop it serves)
    if args.samples_num > 1:
        log_distinct(logger, img_name, finals)
    pick()
    logger.info("total %.2fs" % (time.time() - t0))
    return finals


if __name__ == "__main__":
    main()
