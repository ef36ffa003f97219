/*
 * conzic_hip.h -- C ABI of the MI355X-native ConZIC polishing engine (libconzic_hip.so).
 *
 * Drop-in boundary for ONE path of joeyz0z/ConZIC: the per-position polishing step
 *   mask a position -> BERT masked-LM forward -> softmax/top-K -> K candidate captions ->
 *   CLIP text encode -> cosine vs cached image embedding -> alpha/beta(/gamma) fusion -> argmax
 * i.e. the loop bodies of
 *   gen_utils.py:64-81   (sequential_generation), :114-130 (shuffle_generation),
 *   gen_utils.py:160-179 (span_generation),       :209-226 (random_generation),
 *   control_gen_utils.py:43-65, :98-120           (sentiment_*_generation)
 * plus the once-per-image CLIP vision encode (clip/clip.py:48-62).  Beyond the reference: whole chains on the device
 * (czc_generate*), the scores of finished captions (czc_score_rows: CLIP cosine; czc_fluency_rows: BERT pseudo-log-likelihood)
 * and caption retrieval.
 *
 * The reference is pure Python over torch/transformers, so it has no FFI of its own; the
 * Python modules gen_utils / control_gen_utils / clip.clip / utils at the repo root keep the
 * reference's call surface and bind these entry points through ctypes.
 *
 * Conventions: plain pointers and sizes only (no torch types).  Every function returns an int
 * status (0 = CZC_OK); czc_last_error() gives the message.  One engine per GPU, one host thread
 * per engine, calls are synchronous on return unless noted.  Pointers named *_host must be host
 * memory; pointers named `src`/`dst`/`pixels` may be host OR device memory (hipMemcpyDefault).
 * The engine owns all device memory it allocates; caller buffers stay caller-owned.
 */
#ifndef CONZIC_HIP_H
#define CONZIC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libconzic_hip.so is built with -fvisibility=hidden: the functions declared between this push and its pop are the
 * library's whole dynamic symbol table (tests/test_host_logic.py checks `nm -D`). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define CZC_OK 0
#define CZC_ERR_ARG 1
#define CZC_ERR_HIP 2
#define CZC_ERR_STATE 3
#define CZC_ERR_OVERFLOW 4 /* text bridge scratch overflow (row text > CZC_BRIDGE_MAX_BYTES), or a non-finite CLIP cosine: an fp16
                              quantity overflowed in a tower (options resid16 / refine_rows16 = 0 keep fp32 rows; CZC_PREC_SPLIT) */

#define CZC_PREC_BF16 0 /* throughput mode: CLIP towers on bf16 MFMA operands (fp32 accumulate, residual, LN, */
                        /* softmax); the BERT tower runs on split-fp16 MFMA (hi+lo planes, 3 passes, ~22  */
                        /* mantissa bits) because softmax(logits/0.1) amplifies logit error tenfold and   */
                        /* BERT is only 1.4% of the step's FLOPs                                          */
#define CZC_PREC_F32 1  /* f32-input MFMA everywhere (verification mode, ~1e-6 of the CPU reference) */
#define CZC_PREC_ALL_BF16 2 /* bf16 MFMA in every tower (experiments only) */
#define CZC_PREC_SPLIT 3 /* every tower on split-fp16 MFMA (hi+lo fp16 planes, three passes, ~22 mantissa bits,  */
                         /* fp32 accumulate): fp32-class results at 3/16 of the f32-MFMA cost.  The mode for     */
                         /* checkpoints whose logit_scale.exp() is large (clip/clip.py:95-98: x100 for the       */
                         /* published clip-vit-base-patch32), where a bf16 cosine error would be multiplied by   */
                         /* 100 ahead of softmax_K and leave the 1e-3 fused-score budget                          */

#define CZC_PREC_FP16 4 /* CLIP towers on single-pass IEEE fp16 MFMA: the bf16 kernels with the fp16 opcode and converter */
                        /* (same bytes, same speed), 11 significand bits instead of 8 -> ~8x smaller cosine error: inside  */
                        /* the 1e-3 fused-score budget at the published logit scale (x100) where bf16 is out by 2-3x.  */
                        /* BERT on split-fp16 as in CZC_PREC_BF16.  Operands are bounded (LayerNorm outputs, attention    */
                        /* context, quick-GELU outputs); residual stream / accumulators / softmax / statistics stay fp32  */

#define CZC_BRIDGE_MAX_BYTES 512 /* decoded caption text per candidate row */
#define CZC_CLIP_MAX_LEN 77       /* clip/clip.py:71-72 (max_length = 77, truncation) */
#define CZC_PREC_REFINE 5 /* screen-then-refine, for checkpoints with a large logit scale (published CLIP: x100): all K candidates  */
                         /* through the single-pass fp16 text tower (CZC_PREC_FP16 speed), then the candidates that carry the     */
                         /* softmax_K mass (p_k > theta_x / (beta * exp(logit_scale)), theta_x = 2), the two best fused scores and */
                         /* a mass-stratified sample of the rest (it measures the screening tower's mean error) are re-encoded by */
                         /* the split-fp16 tower and the scores are formed from the mixed cosines: a candidate that keeps its     */
                         /* screening cosine moves its fused score by at most theta_x * |its error - the mean|.  Inside            */
                         /* czc_generate a margin gate skips the second pass where the winner is already certain                   */
                         /* (czc_refine_gate_stats).  Vision tower and BERT: split-fp16.  Options "refine_samples" (12) /           */
                         /* "refine_theta_x1000" (2000) / "refine_gate_x1e6" (400) tune it.  Measured figures: the block below.     */
/*
 * BEGIN GENERATED measured
 * Measured on one MI355X, round 6 (generated by tools/refresh_docs.py from profiles/r06_*):
 *   fused score vs the reference, worst over the full-size goldens: CZC_PREC_BF16 2.46e-04, CZC_PREC_REFINE 2.78e-04,
 *   CZC_PREC_SPLIT 4.2e-06, CZC_PREC_F32 7.3e-06 (bar 1e-3);
 *   CZC_PREC_REFINE against CZC_PREC_SPLIT over 2560 more image-steps: worst 3.80e-04, 99.9th percentile 1.3e-04, winners identical
 *   2560 / 2560; guard sample maximum 1.74e-04 against 2.33e-04 over all candidates;
 *   BASELINE configs[2]: 79.4 captions/s (CZC_PREC_BF16), 67.1 (CZC_PREC_REFINE through czc_generate, 76 % of the image-steps gated).
 * END GENERATED measured
 */
#define CZC_MAX_TOPK 1024
#define CZC_MAX_BERT_LEN 64
#define CZC_MAX_ROWS 16384 /* rows of one czc_generate_rows call */

typedef struct czc_engine czc_engine;

/* Shapes of the three frozen towers the reference loads at demo.py:125-132 / clip/clip.py:11-16. */
typedef struct czc_config {
  /* BertForMaskedLM (HF:bert/modeling_bert.py) */
  int32_t bert_vocab, bert_hidden, bert_layers, bert_heads, bert_inter, bert_max_pos;
  float bert_eps;
  /* CLIP text tower + projection (HF:clip/modeling_clip.py:494-586, :675) */
  int32_t clip_vocab, clip_hidden, clip_layers, clip_heads, clip_inter, clip_max_pos, clip_proj;
  float clip_eps;
  int32_t clip_bos_id, clip_eos_id;
  /* CLIP vision tower + projection (HF:clip/modeling_clip.py:594-656, :674) */
  int32_t vis_hidden, vis_layers, vis_heads, vis_inter, vis_image, vis_patch;
  /* BERT special ids (tokenizer.mask_token_id gen_utils.py:67; vocab['.'] utils.py:55-58; skip set gen_utils.py:75) */
  int32_t pad_id, unk_id, cls_id, sep_id, mask_id, dot_id;
  int32_t precision; /* CZC_PREC_* */
} czc_config;

/* Tables that replace the host string round trip of gen_utils.py:75 (batch_decode) ->
 * clip/clip.py:71-74 (CLIPTokenizer) with an on-device BERT-id -> CLIP-id bridge.
 * Built once on the host from the two tokenizers (conzic_amd/bridge.py). */
typedef struct czc_bridge_tables {
  int32_t bert_vocab;
  const uint32_t* piece_off;  /* [bert_vocab+1] offsets into piece_bytes/piece_class            */
  const uint8_t* piece_bytes; /* UTF-8 of each piece, '##' stripped, NFC + lowercased            */
  const uint8_t* piece_class; /* per byte: bits0-1 class of its char (0 L,1 N,2 other,3 space),  */
                              /*           bit2 = first byte of a char                           */
  const uint8_t* piece_flags; /* [bert_vocab] bit0 special (skipped), bit1 '##' continuation,    */
                              /*              bit2 clean-up removes the space before it          */
  int32_t clip_vocab;
  const int32_t* byte_sym;     /* [256] CLIP id of a byte inside a word                          */
  const int32_t* byte_sym_eow; /* [256] CLIP id of a byte that ends a word ('</w>' suffix)       */
  int32_t n_merges;
  const int32_t* merge_left;  /* [n_merges] BPE merges in rank order: (left,right) -> out        */
  const int32_t* merge_right;
  const int32_t* merge_out;
  int32_t bos_id, eos_id;
} czc_bridge_tables;

/* Hyper-parameters of one generate call: demo.py:55-60 / gen_utils.py:289-292 keyword arguments. */
typedef struct czc_hyper {
  float alpha;       /* weight of BERT fluency probs          (gen_utils.py:77)              */
  float beta;        /* weight of CLIP softmax_K score        (gen_utils.py:77)              */
  float gamma;       /* weight of sentiment softmax_K         (control_gen_utils.py:59)      */
  float temperature; /* lm_temperature                         (gen_utils.py:43-44)           */
  int32_t control;   /* 0 caption path (gen_utils.py:77); 1 sentiment: + gamma*softmax_K(senti) + 0.1*(1-e^repeats) */
                     /* (control_gen_utils.py:59); 2 POS: + gamma*softmax_K(acc/0.1) (control_gen_utils.py:165-169)  */
  int32_t negative;      /* sentiment_ctl == "negative" (sentiments_classifer.py:31-32)         */
} czc_hyper;

/* Outputs of one position-step at parity granularity (every pointer optional / may be NULL).
 * Shapes use B images, K = top_k.  Host or device memory. */
typedef struct czc_step_out {
  float* probs;      /* [B,K] masked softmax probs, descending   (gen_utils.py:45-47) */
  int32_t* idxs;     /* [B,K] their vocab ids                     (gen_utils.py:47)    */
  int32_t* cand_ids; /* [B,K] idxs * token_mask[idxs]             (gen_utils.py:72)    */
  int32_t* clip_ids; /* [B*K, CZC_CLIP_MAX_LEN] bridged CLIP ids  (clip/clip.py:71-74) */
  int32_t* clip_len; /* [B*K] tokens incl. BOS/EOS                                     */
  float* clip_score; /* [B,K] softmax_K(cos * exp(logit_scale))   (clip/clip.py:97)    */
  float* clip_ref;   /* [B,K] cosine                              (clip/clip.py:98)    */
  float* senti_raw;  /* [B,K] control score: sentence sentiment (sentiments_classifer.py:46) or POS-template */
                     /*       match fraction (POS_classifier.py:17-29), by czc_hyper.control                  */
  float* repeats;    /* [B,K] repeat count - 1                    (control_gen_utils.py:53)    */
  float* final_score;/* [B,K] fused score                         (gen_utils.py:77 / control_gen_utils.py:59) */
  int32_t* best;     /* [B]   argmax_K (first max)                (gen_utils.py:78)    */
  float* best_cos;   /* [B]   cosine of the winner                (gen_utils.py:80)    */
  float* logits;     /* [B,V] BERT logits of the masked row       (gen_utils.py:42)    */
} czc_step_out;

/* ---- lifecycle ---------------------------------------------------------------------- */
int czc_create(const czc_config* cfg, int device_id, czc_engine** out_engine);
int czc_destroy(czc_engine* e);
/* A second engine on the same GPU that SHARES `parent`'s resident weights (no copy, no reload) and owns everything
 * else: stream, workspace, image embeddings, token mask / bridge / lexicon / POS tables and the control callback (set
 * them on the replica as on the parent), options (copied at creation), profile.  Images are independent (gen_utils.py:64-81 has no
 * cross-image term), so a host that drives parent and replica(s) from separate threads on disjoint sub-batches gets
 * the same captions image for image while their kernels overlap on the GPU.  `parent` must be finalized and must
 * outlive its replicas; czc_destroy(replica) frees only what the replica owns. */
int czc_replicate(czc_engine* parent, czc_engine** out_engine);
const char* czc_last_error(const czc_engine* e); /* e may be NULL: last create error */
int czc_version(void);

/* ---- frozen state (replaces from_pretrained at demo.py:125-126, clip/clip.py:12-16) ---- */
/* One call per state-dict entry (names and shapes: SURVEY.md §8b).  dtype must be 0 (fp32).
 * `src` may be a device pointer, which is how ranks > 0 hand over weights they received
 * through the RCCL broadcast (bench.py / conzic_amd/dist.py). */
int czc_load_tensor(czc_engine* e, const char* name, int dtype, int ndim, const int64_t* shape, const void* src);
/* After the last czc_load_tensor: checks completeness, fuses q/k/v, ties the MLM decoder to the
 * word embeddings (HF:bert/modeling_bert.py:910-913), converts GEMM operands to the engine precision. */
int czc_finalize_weights(czc_engine* e);
/* token_mask of demo.py:135-143: fp32 [V]; the '.' entry is overridden per step (utils.py:53-59). */
int czc_set_token_mask(czc_engine* e, const float* mask, int vocab);
int czc_set_bridge(czc_engine* e, const czc_bridge_tables* t);
/* Per-BERT-token sentiment score (stand-in for sentiments_classifer.py:9-33). */
int czc_set_lexicon(czc_engine* e, const float* lexicon, int vocab);

/* The same score keyed the way the reference scores (sentiments_classifer.py:14-30: per WORD and coarse POS class,
 * mean of pos_score - neg_score over the word's SentiWordNet synsets): table fp32 [V][5] over the classes
 * 0 '' | 1 n | 2 v | 3 a | 4 r, addressed by a word's FIRST piece ('##' continuations add nothing), and
 * class_of_token uint8 [V] = the class a context-free tagger gives that token (host pointer).  Where nltk and its
 * corpora exist, conzic_amd/sentiment.py fills both from SentiWordNet; table == NULL returns to czc_set_lexicon. */
int czc_set_lexicon_pos(czc_engine* e, const float* table, const uint8_t* class_of_token, int vocab);

/* POS control (control_gen_utils.py:136-195 / POS_classifier.py:6-31): per-BERT-token universal-tagset id
 * (stand-in for nltk.pos_tag) and the template as one bit mask of accepted tag ids per word
 * position (0xFFFF = the reference's "" wildcard; bit 15 = the "" tag that pads a too-short sentence matches as well,
 * POS_classifier.py:19-25 with a string entry); n_template <= 32. */
int czc_set_pos(czc_engine* e, const uint8_t* tag_of_token, int vocab, const uint16_t* template_masks, int n_template);

/* Control scores from the host instead of the tables above: the reference scores every candidate SENTENCE with nltk
 * (sentiments_classifer.py:9-33: word_tokenize -> context-dependent pos_tag -> SentiWordNet; POS_classifier.py:12-29:
 * pos_tag(tagset="universal") against the template), which the per-token tables can only approximate.  With a callback
 * set, every step with czc_hyper.control != 0 calls it once, AFTER the step's CLIP text tower has been queued on the
 * engine's stream and BEFORE the combine kernel that consumes the scores: the host scores while the GPU encodes the
 * candidates (the reference runs the two one after the other, control_gen_utils.py:56-58), so the scorer's wall time only
 * shows where it exceeds the tower's:
 *   inp   int32 [B,T]  the current rows, [MASK] at column gen_idx          (control_gen_utils.py:49-50)
 *   cand  int32 [B,K]  the candidate ids, idxs * token_mask[idxs]           (control_gen_utils.py:52)
 *   scores fp32 [B,K]  out: the raw control score of row b with cand[b][k] at gen_idx -- the sentence sentiment AFTER the
 *                      sign flip of "negative" (sentiments_classifer.py:30-32), or the template match fraction
 *                      (POS_classifier.py:17-29); softmax_K / gamma / the repeat penalty stay in the combine kernel
 * and a non-zero return fails the step with CZC_ERR_STATE.  All pointers are host memory owned by the engine and valid
 * during the call only; the call happens on the thread that called czc_step / czc_generate.  fn == NULL removes it. */
typedef int (*czc_control_fn)(void* user, const int32_t* inp, const int32_t* cand, int B, int T, int K, int gen_idx,
                              float* scores);
int czc_set_control_callback(czc_engine* e, czc_control_fn fn, void* user);

/* ---- once per image: clip/clip.py:48-62 after the image processor ------------------------ */
/* pixels fp32 [B,3,S,S] -> un-normalised image_embeds [B,proj] (out may be NULL).  The engine
 * keeps the L2-normalised embeds resident for the following step/generate calls (the north
 * star's "encode once per image and cache"). */
int czc_encode_images(czc_engine* e, const float* pixels, int B, float* out_embeds);
/* The image processor itself (clip/clip.py:55-56 -> CLIPProcessor -> HF CLIPImageProcessor, PIL backend): RGB uint8
 * [height][width][3] (host or device pointer) -> bicubic resize of the shorter side to S (Pillow's 8-bit resampler,
 * bit-exact) -> centre crop SxS -> /255 -> (x - mean[c]) / std[c] -> CHW fp32, written to slot `slot` of the engine's
 * staged pixel batch on the device (and to pixels_out [3,S,S], host or device, when not NULL).  mean/std: 3 floats. */
int czc_preprocess_u8(czc_engine* e, const uint8_t* rgb, int height, int width, const float* mean, const float* stdv,
                      int slot, float* pixels_out);
/* Region captions: n boxes of ONE image into staged slots slot0 .. slot0 + n - 1 in one call.  boxes int32 [n][4] = x0, y0, x1,
 * y1 (host memory) in PIL's crop convention: pixel coordinates, x1 and y1 exclusive.  Slot slot0 + i holds, bit for bit, what
 * czc_preprocess_u8 writes for the contiguous copy of rgb[y0:y1, x0:x1] (PIL: crop(box), then the processor).  The image is
 * uploaded once; the boxes are read in place through the image's row stride; per chunk of at most option "regions_chunk" boxes
 * the descriptors and the crop windows' coefficient tables travel in one copy, two kernels run over all regions of the chunk
 * and the host synchronises once.  Only what the crop window reads is computed, so a region's intermediate holds at most
 * (source rows its window reads) x S x 3 bytes whatever the box's aspect.  pixels_out: [n,3,S,S], host or device, or NULL.
 * The staged batch grows as in czc_preprocess_u8 and keeps the slots it held.  CZC_ERR_ARG, before any GPU work and with the
 * staged slots untouched: n outside [1, CZC_MAX_REGIONS], slot0 outside [0, 2^20], a box that is empty or leaves the image
 * (PIL would pad with black; the engine refuses), a box whose resized long side int(S * long / short) exceeds 2^24, the
 * size limits of czc_preprocess_u8. */
#define CZC_MAX_REGIONS 1024
int czc_preprocess_regions_u8(czc_engine* e, const uint8_t* rgb, int height, int width, const int32_t* boxes, int n,
                              const float* mean, const float* stdv, int slot0, float* pixels_out);
/* czc_encode_images over staged slots 0..B-1 (no host round trip of the pixels). */
int czc_encode_staged(czc_engine* e, int B, float* out_embeds);
/* Alternative: hand over image_embeds computed elsewhere (fp32 [B,proj], un-normalised). */
int czc_set_image_embeds(czc_engine* e, const float* embeds, int B);

/* clip/clip.py:64-84 after tokenisation: CLIP ids int32 [n, CZC_CLIP_MAX_LEN] (right-padded) and
 * lengths (tokens incl. BOS/EOS) -> un-normalised text_embeds fp32 [n, proj]. */
int czc_encode_text(czc_engine* e, const int32_t* clip_ids, const int32_t* clip_len, int n, float* out_embeds);
/* clip/clip.py:86-98 `compute_image_text_similarity_via_embeddings`: image_embeds [B, proj] and text_embeds [B*K, proj]
 * (both as returned by czc_encode_images / czc_encode_text, un-normalised) -> clip_score [B, K] = softmax over an image's K
 * texts of cos * exp(logit_scale of the loaded checkpoint), clip_ref [B, K] = the cosines.  K <= CZC_MAX_TOPK.  (czc_step /
 * czc_generate never call it: the same arithmetic runs fused inside their score-combine kernel.) */
int czc_similarity(czc_engine* e, const float* image_embeds, const float* text_embeds, int B, int K, float* clip_score,
                   float* clip_ref);

/* ---- the hot path ------------------------------------------------------------------------ */
/* Parity granularity: one position-step (gen_utils.py:66-81) on `inp` int32 [B,T] (in/out, host
 * or device).  gen_idx = seed_len + position; n_mask = how many consecutive positions starting
 * at gen_idx are overwritten with [MASK] before the BERT forward (1 normally, 2 for the first
 * step of a span, 0 = re-use the previous forward, gen_utils.py:164-166); dot_allowed = the
 * update_token_mask rule (utils.py:53-59).  n_mask = 0 needs a previous czc_step / czc_generate forward of the same
 * [B,T]; after an n_mask = 1 step only row gen_idx of that forward exists (option "bert_prune"), so n_mask = 0 at
 * another gen_idx returns CZC_ERR_STATE -- the reference only re-uses a forward after masking two positions
 * (gen_utils.py:164-166), which is n_mask = 2 here and keeps every row. */
int czc_step(czc_engine* e, int32_t* inp, int B, int T, int gen_idx, int n_mask, int dot_allowed, int top_k,
             const czc_hyper* hp, const czc_step_out* out);

/* Throughput granularity: a whole *_generation call with no host round trips except one 8-byte
 * size read per step (option "memo": plus one 16-byte read of the active-image count at the first step of a (position,
 * n_mask) key the call has visited before).  init_ids int32 [T] = `[CLS] prompt [MASK]xL [SEP]` (utils.py:46-51),
 * seed_len = len(prompt.split())+1 (gen_utils.py:56), positions[n_steps] / n_mask[n_steps] as in
 * czc_step, snapshot_every = steps per bookkeeping snapshot (gen_utils.py:82-92).
 * out_ids int32 [n_steps/snapshot_every, B, T], out_cos fp32 [n_steps/snapshot_every, B]
 * (the winner cosine of the snapshot's last step, gen_utils.py:80-81,92). */
int czc_generate(czc_engine* e, int B, int T, int L, int seed_len, const int32_t* init_ids_host, int top_k,
                 int n_steps, const int32_t* positions_host, const int32_t* n_mask_host, int snapshot_every,
                 const czc_hyper* hp, int32_t* out_ids, float* out_cos);

/* czc_generate with a visiting order and an image PER ROW: R rows; row r polishes a caption for image image_of_row[r] (index
 * into the resident embeds of the last czc_encode_images / czc_set_image_embeds; NULL = identity, then R must equal that
 * batch; several rows may name one image) and visits positions[s*R + r] at step s.  Everything else as czc_generate: one
 * init row for all rows, n_mask[n_steps] one value per step for all rows, out_ids int32 [n_steps/snapshot_every, R, T],
 * out_cos fp32 [n_steps/snapshot_every, R].  This is the shape of the reference's sample loop (demo.py:83 / run.py: S calls for
 * S samples of an image, each with a new shuffle / random order, gen_utils.py:110-111, :210) as ONE batch.  The schedule
 * (column and '.' rule of every row and step) is uploaded once; a step reads its slice on the device, so the call has
 * czc_generate's host traffic.  Rows are independent (gen_utils.py:64-81 has no cross-row term): row r returns what a
 * czc_generate call with row r's order returns for its image at the same row count, and a call whose rows all share one order
 * (image_of_row NULL or the identity) returns what czc_generate returns, bit for bit.  The n_mask = 0 re-use rule of czc_step
 * holds per row.  Checked before any GPU work, CZC_ERR_ARG: positions in [0, L), image_of_row inside the resident batch,
 * R <= CZC_MAX_ROWS.  Two limits:
 *   - control callback (czc_set_control_callback): its signature carries one gen_idx, so a controlled call (czc_hyper.control
 *     != 0) with a callback set is accepted only if at every step all rows share one position (it then behaves as in
 *     czc_generate); otherwise CZC_ERR_ARG.
 *     The way out: the control tables (czc_set_lexicon / czc_set_lexicon_pos / czc_set_pos), which work with differing
 *     positions, or one czc_generate call per order.
 *   - option "memo": its keys are (image, position, n_mask) per step group, which a rows call does not have; a rows call
 *     ignores it and czc_memo_stats counts nothing for it.  The rows call has the same rule keyed per row under an option of
 *     its own, "memo_rows" (below; czc_memo_rows_stats), off by default: with it off a rows call runs every step whole. */
int czc_generate_rows(czc_engine* e, int R, int T, int L, int seed_len, const int32_t* init_ids_host,
                      const int32_t* image_of_row_host, int top_k, int n_steps, const int32_t* positions_host,
                      const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp, int32_t* out_ids, float* out_cos);

/* czc_generate_rows with a START ROW per row and steps a row may sit out: infilling (only the blanks of a given caption are
 * polished, the given words stay as context), resume (more sweeps from where an earlier call stopped) and polishing a draft.
 * The reference's CLI never exposed these, but its loop body does them unchanged (gen_utils.py:66 `inp[:, seed_len+ii] = mask`
 * does not care what the rest of the row holds).  Everything not named here is as in czc_generate_rows, which keeps its
 * behaviour bit for bit (as does czc_generate), position -1 refused included.
 *   - init_rows int32 [R, T]: row r starts as init_rows[r].  Ids must lie in [0, bert_vocab); nothing else about their content
 *     is checked -- the caller decides what is prompt, word or [MASK].  Uploaded once; no broadcast.
 *   - positions[s*R + r] == CZC_POS_IDLE: row r does not take part in step s.  Its ids do not change; no BERT row, candidate,
 *     tower row or combine work is spent on it; it is not handed to a control callback; czc_stats, czc_dedup_stats, the
 *     czc_refine_ counters and czc_memo_rows_stats count only the rows that ran.  A step runs on all rows, on none (a step idle
 *     in every row launches nothing) or on a compact batch of the rows that are not idle, with their own columns and '.' rules.
 *     The host knows the schedule, so every step's run list travels with the schedule upload: with option "memo_rows" off an
 *     idle call makes no device-to-host read beyond those of czc_generate_rows.  A call without any idle step runs as
 *     czc_generate_rows does: from the same start row in every row it returns that call's bits.
 *   - groups: n_mask stays one value per step for all rows.  A group is an n_mask >= 1 step plus the n_mask = 0 steps behind
 *     it; a row must be idle for a whole group or for none of it, else CZC_ERR_ARG.  The n_mask = 0 re-use rule of czc_step
 *     keeps holding per row on the compact batches.
 *   - snapshots: out_ids = the rows as they stand; out_cos[snap][r] = the winner cosine of row r's most recent executed step
 *     in this call, 0.0f while it has not executed one (the reference's best_clip_score start value, gen_utils.py:62).
 *   - a step's result depends only on the rows it is given (deterministic argmax; the only state between steps is the
 *     n_mask = 0 re-use inside a group), so resuming from a snapshot of czc_generate / czc_generate_rows with the remaining
 *     positions returns the remaining snapshots of the one long call, bit for bit (CZC_PREC_REFINE places its audit steps by
 *     sweep index within a call, so there the winner cosines of a resumed call may differ in the last bits).  What a compact
 *     batch keeps, and CZC_PREC_SPLIT, are as described for option "memo_rows" below.
 *   - option "memo_rows": an idle step is not a visit -- it neither reads nor replaces the row's entries and is neither a hit
 *     nor a counted row-step.  The active set of a checked step is (not idle) and (miss); CZC_PREC_SPLIT runs a checked step on
 *     every row that is not idle unless all of them hit.  A step at which no row that runs revisits a key needs no check.
 *   - CZC_PREC_REFINE: audit and snapshot rules are unchanged for the rows that run; idle rows are not audited, and an audit
 *     step that is idle in every row is skipped.
 *   - control callback with czc_hyper.control != 0: the rows of a step that are not idle must share one position, else
 *     CZC_ERR_ARG; the callback sees the running rows compacted (B = their count), as under "memo_rows".
 * Checked before any GPU work, CZC_ERR_ARG, and the engine stays usable: a position outside {CZC_POS_IDLE} and [0, L), an id
 * outside the vocabulary, the group rule, and everything czc_generate_rows checks. */
#define CZC_POS_IDLE (-1)
int czc_generate_rows_from(czc_engine* e, int R, int T, int L, int seed_len, const int32_t* init_rows_host,
                           const int32_t* image_of_row_host, int top_k, int n_steps, const int32_t* positions_host,
                           const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp, int32_t* out_ids, float* out_cos);

/* czc_generate_rows_from with a SENTENCE LENGTH per row: captions of different lengths (the reference's --sentence_len, one value
 * per call there) polished in one batch.  Everything not named here is as in czc_generate_rows_from.
 *   - layout: T is the row stride of init_rows / out_ids.  Row r has L_r = len_of_row[r] positions and T_r = seed_len + L_r + 1
 *     tokens ([CLS] prompt, L_r words, [SEP]); columns T_r .. T-1 must hold id 0 ([PAD]) and hold 0 in every snapshot.
 *   - what a row computes: BERT reads exactly the T_r tokens of row r at position embeddings 0 .. T_r-1 and attends over T_r
 *     keys (the reference calls BERT without an attention mask, so padding inside a sequence would be attended to: a shorter
 *     caption runs at its own length instead).  BERT runs on the packed sum of T_r rows of the rows that take part in a step.
 *     The '.' rule of row r is position == L_r - 1; positions lie in {CZC_POS_IDLE} and [0, L_r); a step with n_mask >= 2 at
 *     position p needs p + n_mask <= L_r.
 *   - nothing that reads a row sees its padding: the text bridge (decoding, the repeat count of a candidate the token mask
 *     turned into [PAD], the sentiment sum and the POS word count) stops at T_r.
 *   - rows are independent: row r returns what a czc_generate_rows_from call at T = T_r, L = L_r returns for it, under the
 *     caveats stated there for compact batches -- the form of BERT's GEMMs depends on the packed row count and CZC_PREC_SPLIT's
 *     tower picks kernels by row count, so ids agree and winner cosines may differ in the last bits (1e-6).
 *   - a call whose rows all have T_r == T takes czc_generate_rows_from's path and returns its bits.
 *   - CZC_PREC_REFINE: a row that is idle at a snapshot step returns the cosine its last step left; that step re-encodes a
 *     margin-gated row's winner as a snapshot step does, so the 1e-6 above holds for rows shorter than their companions too.
 *   - option "memo_rows" applies unchanged (rows are compared over the stride T); idle steps, image_of_row and the control
 *     tables work as in czc_generate_rows_from.  The offsets of the full batch and of every step's run list travel with the
 *     one schedule upload; those of a "memo_rows" compact batch are derived on the host from the list it already reads and
 *     uploaded: no device-to-host read beyond czc_generate_rows_from's in either case.
 *   - control callback with czc_hyper.control != 0: accepted only if the rows of a step that are not idle share one position
 *     AND one length; the callback is then told T = T_r and sees the rows' first T_r columns.  Otherwise CZC_ERR_ARG.
 *   - czc_stats' bert_rows counts the sum of T_r over the rows that ran.
 * Checked before any GPU work, CZC_ERR_ARG, and the engine stays usable: len_of_row[r] outside [1, T - seed_len - 1], a position
 * >= L_r, a non-zero id in a row's tail, the n_mask >= 2 overrun, and everything czc_generate_rows_from checks. */
int czc_generate_rows_len(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host, const int32_t* len_of_row_host,
                          const int32_t* image_of_row_host, int top_k, int n_steps, const int32_t* positions_host,
                          const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp, int32_t* out_ids, float* out_cos);

/* czc_generate_rows_len with a czc_hyper PER ROW: one image under every control signal (plain caption, positive, negative, POS
 * template -- the reference's --run_type / --control_type / --sentiment_type, one value per process there), or an alpha / beta /
 * temperature sweep, in one batch.  Everything not named here is as in czc_generate_rows_len: idle steps, image_of_row, ragged
 * lengths, snapshots, option "memo_rows".  top_k, n_mask and the POS template of czc_set_pos stay one value per call.
 *   - len_of_row == NULL: every row has L = T - seed_len - 1 positions (the shape of czc_generate_rows_from).
 *   - what row r computes: row r is polished with hp_of_row[r] -- its own temperature in the masked softmax
 *     (gen_utils.py:43-44), its own alpha, beta and gamma in the fusion (gen_utils.py:77 / control_gen_utils.py:59) and its own
 *     control (0 caption, 1 sentiment, 2 POS) and negative.  The text bridge is handed every control table that is set and
 *     scores a candidate by its row's control; a control == 0 row takes no control score at all.
 *   - rows are independent: row r returns what the same call returns for it when every row carries hp_of_row[r] (the caveats
 *     of compact batches and CZC_PREC_SPLIT are those stated for czc_generate_rows_len).
 *   - a call whose R entries are all equal takes the existing path -- czc_generate_rows_len, or czc_generate_rows_from where
 *     len_of_row is NULL -- with that entry, and returns its bits.
 *   - the [R] array is uploaded once, with the schedule.  A compact batch (idle rows, "memo_rows" hits) gathers the records
 *     of the rows that run by the run list it already has: no device-to-host read beyond those of czc_generate_rows_len.
 *   - option "memo_rows" stays exact: a row's hyper-parameters are constant over the call, so its key -- the masked row --
 *     still determines the outcome.
 *   - CZC_PREC_REFINE: the mass threshold theta / (beta * exp(logit_scale)) and the beta of the margin gate are row r's own,
 *     formed on the device; guard, audit steps and the gate's bound are unchanged.
 *   - control callback (czc_set_control_callback) with any row's control != 0: the host scorer is configured for one signal,
 *     so every row must share control and negative, else CZC_ERR_ARG; the one-position and one-length rules of
 *     czc_generate_rows_len apply; alpha, beta, gamma and temperature may still differ between rows.  The control tables
 *     (czc_set_lexicon / czc_set_lexicon_pos / czc_set_pos) serve rows under different signals.
 * Checked before any GPU work, and the engine stays usable.  CZC_ERR_ARG: a control outside {0, 1, 2}, a temperature that is
 * not finite and > 0, a non-finite alpha, beta or gamma, and everything czc_generate_rows_len checks.  CZC_ERR_STATE, with the
 * messages of czc_step: a control == 1 row without lexicon or callback, a control == 2 row without czc_set_pos or callback. */
int czc_generate_rows_hp(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host,
                         const int32_t* len_of_row_host /* NULL: every row has L = T - seed_len - 1 */,
                         const int32_t* image_of_row_host, int top_k, int n_steps, const int32_t* positions_host,
                         const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp_of_row_host /* [R] */,
                         int32_t* out_ids, float* out_cos);

/* czc_generate_rows_hp with a seeded DRAW of the winner per row: row r may take its winner from softmax_K(final_score / tau)
 * instead of the first argmax (the reference's generate_step has such a branch; its caption path never reaches it).  Under the
 * argmax rule two samples of an image differ only by their visiting order; with a tau and a seed per row, S rows of one image
 * give S reproducible, different captions under any order.  Everything not named here is czc_generate_rows_hp's: ragged
 * lengths, idle steps, image_of_row, per-row czc_hyper, snapshots, control callback and tables.
 *   The draw of a row with 64-bit `seed`, at step s of the call's schedule (0-based), for candidate k in [0, K):
 *     1. x = output word (k & 3) of Philox4x32 with 10 rounds (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 *        0xBB67AE85), key = (seed & 0xffffffff, seed >> 32), counter = (step0 + s, k >> 2, 0, 0).  Counter 0 under key 0
 *        gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
 *     2. u = ((x >> 9) + 0.5) * 2^-23: exact in fp32 and strictly inside the unit interval.
 *     3. g = -logf(-logf(u)).
 *     4. z_k = final_k / tau + g in fp32; a candidate with probs_k == 0 (turned into id 0 by the token mask, or without mass
 *        from BERT) takes z_k = -inf.
 *     5. winner = the first index of the maximum z; with no eligible candidate, the first argmax of final as before.
 *   Write-back into the row's own column, best and best_cos follow the winner unchanged.
 *   - a row's result is a function of its content, its hyper-parameters, its seed and the step counter only: not of its index,
 *     its companions in the batch, compaction, streams or engine replicas.
 *   - draw_of_row == NULL, or every tau == 0: czc_generate_rows_hp itself, bit for bit.  In a mixed call a tau == 0 row returns
 *     what czc_generate_rows_hp returns for it (the caveats are those stated for compact batches and the CZC_PREC_SPLIT /
 *     CZC_PREC_REFINE cosines).
 *   - step0 and resume: call A runs n steps; call B starts from A's last snapshot with the rest of the schedule and
 *     step0 = n, and returns what one call over the whole schedule returns (the resume property of czc_generate_rows_from).
 *   - the [R] array is uploaded once, with the schedule; a compact batch gathers the records through the run list it has.  No
 *     device-to-host read beyond those of czc_generate_rows_hp.
 *   - option "memo_rows": a row with tau > 0 never hits -- its outcome is not a function of its masked row alone -- and always
 *     runs; tau == 0 rows hit as before.  Captions are those of memo_rows = 0.
 *   - CZC_PREC_REFINE: the draw happens in the final combine, never in the screening one.  A tau > 0 row is never margin-gated
 *     (the gate proves an argmax) and takes the full selection.  The cosine returned for a drawn winner that was not re-encoded
 *     is its screening cosine minus the estimated mean error of the screening tower, i.e. within the guard's bound
 *     (czc_refine_guard) of the exact one.  Guard and audit steps are unchanged.
 * Checked before any GPU work, and the engine stays usable.  CZC_ERR_ARG: a tau that is not finite or < 0, step0 + n_steps
 * beyond 32 bits, and everything czc_generate_rows_hp checks. */
typedef struct czc_draw {
  uint64_t seed;  /* the row's own: the Philox key */
  float tau;      /* 0: the row keeps the first argmax */
  uint32_t step0; /* step counter of the call's first step (resume: the steps already run) */
} czc_draw;
int czc_generate_rows_draw(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host,
                           const int32_t* len_of_row_host /* NULL: every row has L = T - seed_len - 1 */,
                           const int32_t* image_of_row_host, int top_k, int n_steps, const int32_t* positions_host,
                           const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp_of_row_host /* [R] */,
                           const czc_draw* draw_of_row_host /* [R], or NULL */, int32_t* out_ids, float* out_cos);

/* The CLIP cosine of BERT-id rows with their images, without leaving the device: row r, decoded as the step decodes it
 * (special tokens and [MASK] dropped; the row stops at T_r = seed_len + len_of_row[r] + 1 tokens), passes the text bridge, the
 * text tower as czc_encode_text runs it (independent sequences, no prefix sharing, the exact tower of the engine precision:
 * split-fp16 on CZC_PREC_REFINE) and the steps' cosine kernel against the normalised embedding of image image_of_row[r] of the
 * resident batch (czc_encode_images / czc_set_image_embeds).  A row's cosine does not depend on its index or companions.
 * `rows` may be host or device memory; out_cos is [R].  An overflow of the bridge's scratch or a non-finite cosine returns
 * CZC_ERR_OVERFLOW as in czc_step.
 * Checked before any GPU work, and the engine stays usable.  CZC_ERR_ARG: an id outside the vocabulary (within a row's T_r
 * tokens), len_of_row[r] outside [1, T - seed_len - 1], image_of_row outside the resident batch (NULL: identity, R must equal
 * the resident batch), R > CZC_MAX_ROWS, T > CZC_MAX_BERT_LEN.  CZC_ERR_STATE without bridge tables or image embeds. */
int czc_score_rows(czc_engine* e, const int32_t* rows /* [R, T] BERT ids, host or device */, int R, int T, int seed_len,
                   const int32_t* len_of_row_host /* NULL: every row has T tokens */,
                   const int32_t* image_of_row_host /* NULL: identity, R == resident batch */, float* out_cos /* [R] */);

/* czc_generate_rows_draw with rows TIED into groups that hold one sentence: W rows of a caption each polish a position of their
 * own from the same current sentence, and all winners are written back together (a block-synchronous sweep: ceil(L / W) serial
 * steps instead of L).  Everything not named here is czc_generate_rows_draw's.
 *   - group_of_row == NULL: czc_generate_rows_draw itself, bit for bit.  Group ids are arbitrary values in [0, R); the rows of
 *     a group need not be contiguous.
 *   - the tie: after every step s, for every group g and every member r that ran at column c_r (not idle), every other member
 *     r' of g gets inp[r'][c_r] = inp[r][c_r].  The rows of a group hold the same ids after every step; each row was computed
 *     from the sentence the group held before the step with its own position masked (n_mask = 1): a Gibbs conditional on the
 *     old values.  One launch per step on the full [R, T] batch, behind whatever the step did (in-place run, compact batch with
 *     scatter, "memo_rows" fill); the group table (CSR of member rows) is uploaded once with the schedule.
 *   - out_cos changes meaning: out_cos[snap][r] is the czc_score_rows cosine of the caption as it stands at the snapshot (a
 *     row's winner cosine is that of "old sentence with one word replaced", which never exists once W winners are merged).  It
 *     is computed once per group, on the group's lowest-numbered row, and written to every member; only at snapshot steps and
 *     only when out_cos != NULL.  out_ids is unchanged.  Singleton groups: the ids of czc_generate_rows_draw and cosines that
 *     agree with its within the precision's bound for one sentence in another packing.
 *   - hyper-parameters and draw records may differ between members.  Give members different seeds: the Philox counter is
 *     (step, candidate), so equal seeds would give equal noise at different positions.
 *   - option "memo_rows" applies unchanged: the key is the whole masked row, so a sibling's write makes a miss exactly when it
 *     must, and a row that hit still hands its restored winner to its siblings.  Captions equal those of memo_rows = 0.
 *   - a control callback: the one-position rule of czc_generate_rows_from refuses blocks wider than one; the tables work.
 *   - CZC_PREC_REFINE: gate, audit and guard are as for the rows that run; the snapshot score uses the split tower.
 * Checked before any GPU work, CZC_ERR_ARG, and the engine stays usable: a group id outside [0, R); members of a group that
 * differ in start row, in len_of_row or in image_of_row (NULL is the identity, so it only admits singleton groups); two members
 * of a group that run at the same position in one step; any n_mask other than 1 (the n_mask = 0 re-use of a forward across a
 * tie is not defined, so span order is refused); and everything czc_generate_rows_draw checks. */
int czc_generate_rows_tied(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host,
                           const int32_t* len_of_row_host /* NULL: every row has L = T - seed_len - 1 */,
                           const int32_t* image_of_row_host, const int32_t* group_of_row_host /* [R], or NULL */, int top_k,
                           int n_steps, const int32_t* positions_host, const int32_t* n_mask_host, int snapshot_every,
                           const czc_hyper* hp_of_row_host /* [R] */, const czc_draw* draw_of_row_host /* [R], or NULL */,
                           int32_t* out_ids, float* out_cos);

/* czc_generate_rows_tied with every row also scored against RIVAL images, for captions that tell an image from its look-alikes.
 * Row r has its own image i0 = image_of_row[r] and up to M rivals i1..im of the resident batch.  For candidate sentence t the
 * step forms, next to the one cosine it forms today,
 *     disc = softmax over {i0, i1..im} of exp(logit_scale) * cos(t, ij), taken at i0  =  1 / (1 + sum_j exp(s * (cj - c0)))
 * -- the probability that the caption retrieves its own image among the set -- in fp32, with max(0, max_j s (cj - c0))
 * subtracted before any expf, and adds delta_of_row[r] * disc to the candidate's fused score, last, behind the control terms.
 * The winner (argmax or draw), the write-back and the returned cosine follow as before; c0 has the bits of the step's cosine.
 * Everything not named here is czc_generate_rows_tied's.
 *   - no rivals: rival_of_row == NULL, or every delta 0, or no filled slot: czc_generate_rows_tied itself, bit for bit.  In a
 *     mixed call a row with delta = 0 or without a rival skips the term entirely and returns what that call returns for it.
 *   - rival_of_row is [R, M], indices into the resident image batch, -1 = empty slot, the filled slots first.  It and the
 *     deltas are uploaded once, with the schedule; a compact batch (option "memo_rows", idle rows) gathers them through its run
 *     list as it gathers the hyper-parameters.  The indices always point into the whole resident batch, while the rows' own
 *     embeddings are the gathered per-row copy.
 *   - a row's result depends on its content, hyper-parameters, draw record, own image and rival images only: not on its index,
 *     its companions, the order of its rivals (beyond the rounding of the fp32 sum), compaction or streams.
 *   - option "memo_rows" is exact and unchanged: the rivals of a row do not change during a call.
 *   - tied groups: members may carry different rivals and deltas; out_cos keeps its tied meaning.
 *   - control callbacks and tables behave as for czc_generate_rows_tied.
 *   - CZC_PREC_REFINE: the selection and guard bounds were derived for the softmax-K term alone.  A call on that engine with
 *     any row where delta != 0 and a slot is filled is refused with CZC_ERR_STATE and a message that names the CZC_PREC_SPLIT
 *     engine (conzic_amd.runtime obtains one, as the guard's rerun does).  czc_score_rows_vs works on every precision: it uses
 *     the exact tower, as czc_score_rows does.
 * Checked before any GPU work, CZC_ERR_ARG, and the engine stays usable: M outside [1, CZC_MAX_RIVALS] when the array is
 * given; an index outside [-1, resident batch); a rival equal to the row's own image; a filled slot behind an empty one; a
 * delta that is not finite; clip_proj * CZC_MAX_RIVALS * 4 beyond the kernel's 32 KB LDS array (clip_proj > 512); and everything
 * czc_generate_rows_tied checks. */
#define CZC_MAX_RIVALS 16
int czc_generate_rows_vs(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host,
                         const int32_t* len_of_row_host /* NULL: every row has L = T - seed_len - 1 */,
                         const int32_t* image_of_row_host, const int32_t* group_of_row_host /* [R], or NULL */, int top_k,
                         int n_steps, const int32_t* positions_host, const int32_t* n_mask_host, int snapshot_every,
                         const czc_hyper* hp_of_row_host /* [R] */, const czc_draw* draw_of_row_host /* [R], or NULL */,
                         const int32_t* rival_of_row_host /* [R, M] indices into the resident image batch, -1 = none; or NULL */,
                         int M, const float* delta_of_row_host /* [R] */, int32_t* out_ids, float* out_cos);
/* czc_score_rows, then the rival kernel at K = 1: out_cos [R] has the bits czc_score_rows returns, out_disc [R] is the disc of
 * czc_generate_rows_vs for the row as it stands (1 for a row without rivals, and everywhere with rival_of_row == NULL).
 * Either output pointer may be NULL.  The checks of czc_score_rows and, for the table, those of czc_generate_rows_vs. */
int czc_score_rows_vs(czc_engine* e, const int32_t* rows /* [R, T] BERT ids, host or device */, int R, int T, int seed_len,
                      const int32_t* len_of_row_host, const int32_t* image_of_row_host, const int32_t* rival_of_row_host, int M,
                      float* out_cos /* [R] */, float* out_disc /* [R] */);

/* czc_generate_rows_vs with a VOCABULARY SET per row: "never say these words for this image", "describe it with words from this
 * list only", "sample 3 may not re-use the nouns of samples 1 and 2", or one image under a plain and a restricted vocabulary side
 * by side, in one batch instead of one czc_set_token_mask and one call per variant.  Everything not named here is
 * czc_generate_rows_vs': ragged lengths, idle steps, image_of_row, hyper-parameters, draws, tied groups, rivals, snapshots.
 *   - the sets are bitsets: sets is uint32 [n_sets, W], W = ceil(bert_vocab / 32); bit (i & 31) of word (i >> 5) is 1 when id i
 *     is allowed.  Bits at or above bert_vocab in the last word are ignored.  set_of_row is [R]; -1 = the row has no set.
 *   - the rule: in the masked softmax of a row r with set s (gen_utils.py:42-47) the mask factor of id i is
 *         mk(i) = (i == dot_id) ? the '.' rule of the row : token_mask[i] * bit_s(i).
 *     Nothing else changes: no renormalisation after masking, the ascending-id tie rule, cand = id * mk -- an id the set removed
 *     becomes [PAD] with probability 0, exactly as a stop word does.  The '.' rule overrides the set as it overrides the token
 *     mask (utils.py:53-59).  Only the top-K kernel knows about sets.
 *   - E, the defining property: a call whose rows all carry set s returns, bit for bit (ids and cosines, every precision), what
 *     the same call without sets returns after czc_set_token_mask(token_mask * bits_s).  Rows are independent: in a mixed call
 *     row r returns what the call returns when every row carries row r's set (under the compact-batch caveats stated for
 *     czc_generate_rows_len); a row with -1 returns what it returns today.
 *   - set_of_row == NULL, or every entry -1: czc_generate_rows_vs itself, bit for bit.
 *   - an all-zero set is legal: the row proposes [PAD] and possibly '.', which is what E says.  So is an allow-list shorter than
 *     top_k (conzic_amd.runtime refuses that one, because [PAD] winners surprise users).
 *   - the bitsets and the indices are uploaded once, with the schedule.  A compact batch (idle rows, ragged lengths, "memo_rows"
 *     hits) gathers the indices of the rows that run through the run list it already has, as it gathers the hyper-parameters;
 *     the table of bitsets stays where it is.  No device-to-host read beyond those of czc_generate_rows_vs.
 *   - option "memo_rows" stays exact: a row's set is constant over the call, so its key still determines the outcome.
 *   - CZC_PREC_REFINE: nothing changes; selection, gate and guard work on whatever candidates the top-K kernel produced.
 *   - czc_step, czc_generate and option "memo" take no sets.
 * Not built: sets per position; required ("must appear") words; a per-row top_k; any eligibility rule in the fusion -- a [PAD]
 * candidate can still win, as today; the exact host scorer for mixed sets -- the control-callback rules of czc_generate_rows_vs
 * apply unchanged.
 * Checked before any GPU work, CZC_ERR_ARG, and the engine stays usable: n_sets < 1 with a set_of_row array; n_sets >
 * CZC_MAX_VOCAB_SETS (4096 sets = 15 MB at bert_vocab = 30 522); an index outside [-1, n_sets); sets == NULL with an index >= 0;
 * and everything czc_generate_rows_vs checks. */
#define CZC_MAX_VOCAB_SETS 4096
int czc_generate_rows_vocab(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host,
                            const int32_t* len_of_row_host /* NULL: every row has L = T - seed_len - 1 */,
                            const int32_t* image_of_row_host, const int32_t* group_of_row_host /* [R], or NULL */, int top_k,
                            int n_steps, const int32_t* positions_host, const int32_t* n_mask_host, int snapshot_every,
                            const czc_hyper* hp_of_row_host /* [R] */, const czc_draw* draw_of_row_host /* [R], or NULL */,
                            const int32_t* rival_of_row_host /* [R, M], or NULL */, int M, const float* delta_of_row_host /* [R] */,
                            const uint32_t* sets_host /* [n_sets, W] */, int n_sets, const int32_t* set_of_row_host /* [R] or NULL */,
                            int32_t* out_ids, float* out_cos);

/* Caption fluency: BERT's pseudo-log-likelihood of finished rows, on the device -- the BERT-side twin of czc_score_rows.
 * Lmax = T - seed_len - 1.  Row r has L_r = len_of_row[r] words at columns seed_len .. seed_len + L_r - 1 and T_r = seed_len + L_r + 1
 * tokens.  For every word j < L_r BERT reads the row's T_r tokens with word j masked, as a step reads them (position embeddings
 * 0 .. T_r - 1, attention over its own T_r keys, no padding seen; the engine's BERT precision; option "bert_prune" applies), and
 *   out_logp[r][j] = log softmax(logits / temperature) at the id the row holds at word j (natural log),
 *   out_rank[r][j] = #{i : x_i > x_t} + #{i < t : x_i == x_t} on the raw logits x, t that id: its place in the step's sorted
 *                    candidate list under an all-ones token mask (ties in ascending id, the top-K kernel's rule),
 *   out_pll[r]     = out_logp[r][0] + ... + out_logp[r][L_r - 1], summed in that order in fp32.
 * Columns j >= L_r hold 0.0f and -1.  Any output pointer may be NULL, but not all three.
 * Prompt, [CLS] and [SEP] are context and are never scored; an id is scored as it stands (a [MASK] left in a row is scored as
 * the id mask_id); the token mask plays no part -- this is BERT's distribution, not the step's masked one.
 * The N = sum L_r masked sequences run in chunks of at most "fluency_chunk" (cut at any sequence boundary; ragged rows where the
 * lengths differ, dense rows where every T_r == T).  One upload of the call's tables, one read of the results at the end.  A
 * position's result is a function of its row's content, its length and the temperature; across companions, chunk sizes and row
 * orders it agrees within the engine precision (the form of BERT's GEMMs depends on the packed row count, as for
 * czc_generate_rows_len), and the same call repeated returns the same bits.
 * Needs finalized weights only: no bridge tables, no image embeds, no token mask.  Leaves the resident image embeds, the text
 * index, the options, the memo and the counters of czc_stats alone.  It ends any forward re-use: an n_mask = 0 czc_step right
 * after it returns CZC_ERR_STATE.
 * Checked before any GPU work, CZC_ERR_ARG, and the engine stays usable: R outside [1, CZC_MAX_ROWS], T outside
 * [1, CZC_MAX_BERT_LEN], seed_len < 0, T - seed_len - 1 < 1, a length outside [1, Lmax], an id outside the vocabulary within a
 * row's T_r tokens, a temperature that is not finite and > 0, all outputs NULL.  CZC_ERR_STATE without finalized weights.
 * CZC_ERR_OVERFLOW when a log-probability is not finite. */
int czc_fluency_rows(czc_engine* e, const int32_t* rows /* [R, T] BERT ids, host or device */, int R, int T, int seed_len,
                     const int32_t* len_of_row_host /* NULL: every row has L = T - seed_len - 1 */, float temperature,
                     float* out_logp /* [R, Lmax] */, int32_t* out_rank /* [R, Lmax] */, float* out_pll /* [R] */);

/* Engine options (all are exact work reductions / kernel choices; results agree within the engine precision):
 *   "share_prefix"    (1) encode the causal prefix common to an image's K candidates once per step instead of K
 *                         times
 *   "dedup"           (1) with "share_prefix": candidates of one image whose CLIP id rows are identical (all the candidates the
 *                         token mask turned into [PAD], gen_utils.py:72-75) are encoded once and share one feature
 *                         (czc_dedup_stats)
 *   "bert_prune"      (1) n_mask == 1 steps: the last BERT layer behind its attention (out-projection, LayerNorms, MLP) on the
 *                         masked row of every sequence only -- the one row the MLM head reads (gen_utils.py:69)
 *   "bert_fuse_splitk_ln" (1) BERT fc2 (split along K at every row count above 32): the LayerNorm kernel behind it sums the slice slabs,
 *                         bias and residual itself instead of a reduce kernel followed by the LayerNorm kernel; bit-identical
 *   "pack_branches"   (1) attention of the branch rows with G candidates packed per 32-query MFMA tile
 *   "pool_last_layer" (1) last CLIP-text layer: out-projection + MLP on the EOS rows only
 *   "share_layer0"    (1) CLIP-text layer 0, on the folded path ("resid16" + "fold_ln") wherever the per-image branch attention
 *                         kernel serves the step: the input of a packed row there is token_embedding[id] + position_embedding[pos],
 *                         so q / k / v are formed once per distinct (id, position) row of an image and the branch attention fetches
 *                         its rows through an index table; bit-identical
 *   "pool_last_qkv"   (1) with "pool_last_layer", on the folded path ("resid16" + "fold_ln") wherever the per-image branch attention
 *                         kernel serves the step: the last layer also forms q and the attention context on the EOS rows only
 *                         (k / v of all rows; no trunk attention); bit-identical
 *   "fold_ln"         (1) with "resid16": the LayerNorms inside the CLIP-text stack folded into the q/k/v and fc1 GEMMs (they
 *                         multiply x itself on the fp16 MFMA by weights whose rows carry the gain and are centred, and scale with
 *                         the row's rstd, which comes from partial sums the producer GEMMs leave): no LayerNorm kernel and no
 *                         normalised copy of the rows; 0 = LayerNorm kernels
 *   "fuse_ln"         (1) fp32-residual CLIP-text tower (fp16 / refine engines; bf16 with resid16 = 0) at >= 8192 packed rows: the out-projection runs as a full-row
 *                         kernel that also emits LN2 of its result (no LayerNorm pass for it); 2 = fc2 -> the next
 *                         layer's LN1 as well (measured slower), 0 = off
 *   "resid16"         (1) residual stream of the CLIP-text tower as IEEE fp16 rows in HBM (fp32 accumulate, bias and residual
 *                         add; one rounding per update): 1 = the bf16 engine (CZC_PREC_BF16), 2 = the single-pass fp16 tower too
 *                         (outside its validated error budget: experiments), 0 = fp32 rows everywhere.  With it the
 *                         out-projection runs on the weight-stationary kernel ("fuse_ln" then has nothing to fuse)
 *   "refine_theta_gen_x1000" (4000): the same threshold inside czc_generate (ids and winner cosines are its output, not the K scores)
 *   "refine_samples" (12) / "refine_samples_step" (24), "refine_theta_x1000" (2000): CZC_PREC_REFINE selection -- strata of the
 *                         mass-stratified sample inside czc_generate / in czc_step, and the softmax_K mass threshold
 *                         theta = value / 1000 / (beta * exp(logit_scale))
 *   "refine_guard_x1e6" (200): trip point of czc_refine_guard, in units of 1e-6 of cosine
 *   "refine_gate_x1e6" (400): cosine-error bound delta of the margin gate of czc_generate (czc_refine_gate_stats), 0 = off
 *   "refine_rows16"   (1) CZC_PREC_REFINE inside czc_generate: the screening pass on the 2-byte residual stream with the folded
 *                         LayerNorms (the "resid16" + "fold_ln" tower form on fp16 operands); gate bound and guard trip point
 *                         are multiplied by "refine_rows16_x1000" / 1000 (1750) while it is on and the selection's mass threshold
 *                         divided by it.  czc_step is not affected
 *   "memo"            (0) czc_generate only: exact step memo.  A step at position p with n_mask = m >= 1 sees, per image b, the
 *                         masked row R(b) = the row with columns seed_len+p .. seed_len+p+m-1 set to [MASK] (what BERT reads).
 *                         Key (b, p, m): the entry holds R(b) from the image's last visit of the key in this call, the winner
 *                         id(s) and cosine(s) that visit produced.  An image whose R(b) equals its entry bit for bit (whole row,
 *                         no hashing) HITS: it does not run, takes the stored winner(s) back (for m = 1 a no-op) and the stored
 *                         cosine.  The polishing rule is a deterministic argmax (gen_utils.py:66-79) and an image's result does
 *                         not depend on the other images of the batch, so the outcome is the one the step would compute.  Span
 *                         order (m = 2 then m = 0, gen_utils.py:160-179): the m = 0 step re-uses the m = 2 forward, hits exactly
 *                         when its m = 2 step hit, and the m = 2 entry holds both winners and cosines.  Sequential, shuffle and
 *                         random orders are all m = 1 keyed by position.  The memo lives for one call (cleared at its start;
 *                         czc_step is not affected).  The first visit of a key runs every image (no check); a later visit runs a
 *                         check kernel, reads the active count, and runs the step as without the memo (all active), not at all
 *                         (none: no BERT, no tower, no combine) or on a compact batch of the active images.  What the compact
 *                         batch keeps: the CLIP-text tower gives every row the same bits at any row count, and a branch longer
 *                         than 32 rows among the skipped images still sends the launch to the per-segment attention kernel as
 *                         the full batch would; BERT below 33 rows runs on the K-split skinny kernel (1e-6 relative on the
 *                         fluency probabilities, 1e-8 on the fused score: an id could only move on a fused-score tie that
 *                         close, the batch coupling the engine already has).  CZC_PREC_SPLIT: its text tower chooses GEMM forms by
 *                         row count (last bits of a cosine), so it runs a step whole unless every image hits.  CZC_PREC_REFINE: audit steps and steps
 *                         whose winner cosine the call returns (snapshot steps with out_cos) never hit -- the guard keeps seeing
 *                         every image, and that cosine comes from a split re-encode whose last bits can depend on which other
 *                         candidates were re-encoded with the winner (gated: the winner alone; full selection: ~20 per image).
 *                         Elsewhere only ids are output.  One case stays theoretical: the last visit took the full selection and
 *                         this one would have been gated; the two winners agree whenever the gate's bound holds, which the guard
 *                         polices.  A control callback (czc_set_control_callback) is called for the images that run only: B is
 *                         the active count and the rows are compacted, so it must be a pure function of its rows (the
 *                         reference scorer is).  Replicas (czc_replicate) inherit the option and keep memos of their own.
 *                         czc_memo_stats counts the hits; czc_stats / czc_refine_gate_stats keep counting what ran
 *   "memo_rows"       (0) czc_generate_rows / czc_generate_rows_from only (czc_generate ignores it; independent of "memo", which a rows call ignores):
 *                         the rule of "memo" keyed per ROW.  n_mask is one value per step for all rows, so the step groups (one
 *                         n_mask >= 1 step plus the n_mask = 0 steps behind it) are shared; the positions are row r's own.  Row
 *                         r's key at a group: its position at every step of the group and the group's n_mask list.  Its entry
 *                         sits in slot (r, first position of the group) -- at most L slots per row -- under a signature word
 *                         (n_mask, group length, column of the second step) and a valid word cleared at the start of the call: a
 *                         first visit, or a visit of the same first position under another group shape, is a miss, and every
 *                         visit replaces the entry.  A row whose masked row R(r) equals its entry (whole row, no hashing) hits:
 *                         it does not run and takes the stored row(s) and cosine(s) back.  A group longer than two steps, or one
 *                         that does not start with n_mask >= 1, never hits.  The host knows the schedule: a step at which no row
 *                         revisits a key (the whole first sweep) runs without a check; otherwise a check (one thread per row,
 *                         R / 256 work-groups) and one read of the active count and the ascending active list, then the step runs
 *                         on all rows, on none, or on a compact batch of the active rows with their own columns and '.' rules.
 *                         The n_mask = 0 re-use rule of czc_step keeps holding per row on a compact batch.  What a compact
 *                         batch keeps, CZC_PREC_SPLIT (a step is skipped only when every row hits) and CZC_PREC_REFINE (audit
 *                         steps and steps whose cosine the call returns never hit) are as for "memo".  A control callback is
 *                         called for the rows that run, compacted (a rows call accepts one only when all rows share a position
 *                         per step).  Entry storage of a call: L x R x T x 12 bytes + L x R x 24 bytes on the device, i.e.
 *                         8 MB + 1 MB at R = 4096, L = 10, T = 16 and, at its largest (R = CZC_MAX_ROWS, L = 62, T = 64), 780 MB + 24 MB,
 *                         kept in the engine's workspace.  Replicas inherit the option and keep entries of their own.
 *                         czc_memo_rows_stats counts the hits
 *   "fluency_chunk"   (1024) czc_fluency_rows: masked sequences per BERT forward, 1 .. 16384 (CZC_ERR_ARG outside); the logits
 *                         buffer of a call holds chunk x vocab x 4 bytes
 *   "regions_chunk"   (64) czc_preprocess_regions_u8: boxes per upload and launch pair, 1 .. 1024 (CZC_ERR_ARG outside); bounds
 *                         the scratch of a call, changes no bit of the result */
int czc_set_option(czc_engine* e, const char* name, int value);
/* Reads an option back (same names and units as czc_set_option), plus three read-only derived values:
 *   "refine_guard_generate_x1e6" / "refine_gate_generate_x1e6": the guard's trip point / the margin gate's bound in force inside
 *       czc_generate (the base values x "refine_rows16_x1000" / 1000 while its screening pass runs on fp16 rows);
 *   "has_folded_ln_weights": 1 when czc_finalize_weights built the folded-LayerNorm operands (it does where an option can use
 *       them: bf16 engine with resid16 >= 1, refine engine with refine_rows16, fp16 engine with resid16 = 2; turning such an
 *       option on afterwards returns CZC_ERR_STATE). */
int czc_get_option(czc_engine* e, const char* name, int* value);

/* ---- caption retrieval ------------------------------------------------------------------- */
/* A resident index of text embeddings and its search: "which of these n known captions is closest to this image?"  One launch
 * scores Q images against the n rows (split-fp16 MFMA, three passes, fp32 accumulation: cosines within 2e-6 of fp64) and keeps
 * the best k per image; the [Q, n] score matrix is never formed.  The search is the same in every engine precision. */
#define CZC_INDEX_MAX_K 64
/* fp32 [n, clip_proj] text embeddings, un-normalised, host or device pointer.  Replaces the engine's index; embeds == NULL or
 * n == 0 drops it.  Rows are L2-normalised on the device.  A row whose norm is 0 or not finite -> CZC_ERR_ARG (one flag read at
 * set time, none on the search path) and the previous index stays.  clip_proj must be a multiple of 32 and at most 1024
 * (CZC_ERR_ARG otherwise); n is limited by int32 ids (2^31 - 2^18 rows) and by memory (4 bytes per element; CZC_ERR_HIP with a
 * message when the allocation fails).  The index belongs to this engine: czc_destroy frees it, czc_replicate does not copy it. */
int czc_index_set(czc_engine* e, const float* embeds, int64_t n);
int czc_index_size(czc_engine* e, int64_t* n);
/* Q images against the index.  image_embeds fp32 [Q, clip_proj] un-normalised (host or device); NULL = the engine's resident
 * image embeddings (czc_encode_images / czc_set_image_embeds), the first Q of them.
 * out_ids int32 [Q, k], out_cos fp32 [Q, k] (host): per image the k rows of largest cosine, ordered by (cosine descending, id
 * ascending).  With fewer than k rows the tail is id -1, cosine -inf.  The cosine of an (image, row) pair has the same bits
 * wherever the row sits in the index, whatever Q, n and option "index_groups" are; identical rows tie and come back lowest id
 * first.  No index -> CZC_ERR_STATE; k < 1 or k > CZC_INDEX_MAX_K, Q < 1, a zero / non-finite query row -> CZC_ERR_ARG.
 * Option "index_groups" (0): work-groups of the scan, 0 = chosen by the launcher, 1..1024 taken as given. */
int czc_index_search(czc_engine* e, const float* image_embeds, int Q, int k, int32_t* out_ids, float* out_cos);

/* ---- measurement ------------------------------------------------------------------------- */
/* HIP-event timing of kernel classes on the engine's own stream (bench.py roofline leg).  on: 0 off, 1 an event pair
 * around every kernel class (3 % slower at B = 256, 37 % at B = 1), 2 only around the CLIP-text tower's classes: its
 * linear layers "gemm_clip_text" / "gemm_clip_refine" (the roofline family), "attention_clip_text" (flops = 4 * hidden *
 * causal (query, key) pairs per layer) and "rowops_clip_text" (embedding, LayerNorm, gathers).
 * kind: those four | "gemm_bert" | "gemm_vision" | "attention" (BERT, vision) | "rowops" (BERT, vision, head) | "topk" |
 * "bridge" | "combine" */
int czc_profile_enable(czc_engine* e, int on);
int czc_profile_reset(czc_engine* e);
int czc_profile_get(czc_engine* e, const char* kind, double* total_ms, int64_t* launches, double* flops);
/* Start / end (ms) of every launch of class `kind` since czc_profile_reset(e), on the clock whose zero is
 * czc_profile_reset(ref) (ref == e for a single engine).  For engines that ran concurrently the host takes the union
 * of their intervals = the time the GPU spent on that class.  Fills at most `cap` pairs; *n = number available. */
int czc_profile_intervals(czc_engine* e, czc_engine* ref, const char* kind, double* start_ms, double* end_ms, int cap,
                          int* n);
int czc_sync(czc_engine* e);
/* counters of the last generate/step: rows pushed through the CLIP text tower etc. */
int czc_stats(czc_engine* e, int64_t* clip_rows, int64_t* clip_seqs, int64_t* bert_rows, int64_t* steps);
/* Exact de-duplication (option "dedup", default 1): of the *clip_seqs candidate sequences the text tower was asked for since
 * czc_profile_reset, *dedup_seqs had a CLIP id row identical to an earlier candidate of the same image (every candidate the
 * token mask turned into [PAD] decodes to the same caption without the word, gen_utils.py:72-75) and were not encoded
 * again: they take their representative's feature bit for bit (f32 engine: exactly what their own rows would have produced;
 * MFMA engines: within the attention tile's packing noise of it, tests/test_step_gpu.py::test_dedup_is_exact). */
int czc_dedup_stats(czc_engine* e, int64_t* dedup_seqs, int64_t* clip_seqs);
/* CZC_PREC_REFINE engines: candidate sequences / packed rows re-encoded by the split-fp16 tower since czc_profile_reset
 * (of the clip_seqs / clip_rows the screening pass saw); zero for the other precisions. */
int czc_refine_stats(czc_engine* e, int64_t* refine_seqs, int64_t* refine_rows);
/* CZC_PREC_REFINE engines, runtime guard of the 1e-3 bound: candidates that keep their screening (single-pass fp16) cosine
 * carry its error minus the estimated mean, and move their fused score by at most theta_x * |that| (theta_x = 2).  Every step
 * that runs the full selection records, over the ~20 candidates per image it re-encodes exactly, the largest
 * |screening error - mean| (*max_dev, since the last reset) and counts the image-steps where it exceeds option
 * "refine_guard_x1e6" * 1e-6 (default 200) in *tripped.  The candidates that are NOT re-encoded reach at most twice the sample
 * maximum on the validated towers (tools/refine_validate.py prints the ratio: 1.15-1.54 on ten plain weight draws, 2.02 on a x6
 * outlier tower), so below the trip point a KEPT candidate moves its own score by at most theta_x * 2 * 2.0e-4 = 8e-4.  That is
 * not the whole error of czc_step: the sample's estimate of the mean screening error is itself uncertain, what is left of the
 * mean scales the softmax denominator, and every RE-ENCODED candidate moves by beta * p_k * exp(logit_scale) * (kept mass) *
 * (error of the mean) -- the largest term on peaky images, measured not bounded: worst |d final_score| against the all-split
 * engine over eleven weight draws 4.5e-4 .. 9.2e-4 with 12 strata, 2.8e-4 .. 5.4e-4 with the 24 czc_step uses since round 6
 * ("refine_samples_step"; czc_generate keeps 12: only the winner matters there).  A checkpoint whose activations the fp16 tower
 * carries worse trips the guard, and
 * conzic_amd/runtime.py then repeats the call on the all-split engine (CZC_REFINE_GUARD=rerun | warn | off).  Inside czc_generate
 * gated image-steps re-encode nothing and are not measured: the audit steps (czc_refine_gate_stats) are. */
int czc_refine_guard(czc_engine* e, int reset, float* max_dev, int64_t* tripped);
/* Option "memo": image-steps of czc_generate calls made with the memo on since czc_profile_reset (*image_steps, B per step), of
 * which *hit_image_steps took a memo entry instead of running (CZC_PREC_SPLIT: only steps on which every image hits).  Zero with
 * the option off. */
int czc_memo_stats(czc_engine* e, int64_t* hit_image_steps, int64_t* image_steps);
/* Option "memo_rows": row-steps of czc_generate_rows calls made with the option on since czc_profile_reset (*row_steps, R per
 * step), of which *hit_row_steps took their entry instead of running (CZC_PREC_SPLIT: only steps on which every row hits).
 * Zero with the option off; czc_memo_stats stays zero for rows calls. */
int czc_memo_rows_stats(czc_engine* e, int64_t* hit_row_steps, int64_t* row_steps);
/* CZC_PREC_REFINE engines, margin gate of czc_generate: a whole *_generation call returns the winner's id of every step and
 * the winner's cosine at the snapshot steps (gen_utils.py:78-81, :92), not the K fused scores.  An image-step whose screening
 * (single-pass fp16) winner stays the winner under EVERY assignment of cosine errors |d_k - common| <= delta (delta = option
 * "refine_gate_x1e6" * 1e-6, default 400 = 2x the largest deviation measured over 256 k candidates; the check is the
 * adversarial one: winner's logit down, challenger's up, the rest both ways) needs no second pass for its id; at a snapshot
 * step its winner alone is re-encoded, for the cosine the call returns.  Image-steps that fail the gate take the full selection,
 * and so does every image at the snapshot step of every fourth sweep (the first included) -- whether or not the caller passes
 * out_cos -- and, in a call too short to reach a snapshot step, at its last step: the audit steps on which the guard above keeps
 * measuring the screening tower.  The gate is the guard's dependant: with "refine_guard_x1e6" = 0 nothing polices the bound the
 * gate rests on and nothing is gated.
 * czc_step never gates: all K scores are its output and all of them are refined.  *gated of *image_steps since
 * czc_profile_reset. */
int czc_refine_gate_stats(czc_engine* e, int64_t* gated, int64_t* image_steps);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CONZIC_HIP_H */
