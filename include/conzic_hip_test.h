/*
 * conzic_hip_test.h -- kernel-level parity hooks of the MI355X-native ConZIC engine (libconzic_hip_test.so).
 *
 * TEST INFRASTRUCTURE, not part of the drop-in boundary: each czc_test_* call runs ONE kernel family of
 * libconzic_hip.so on host data so that tests/ (-m gpu) can compare it with the CPU oracle, czc_bench_gemm is the GEMM
 * microbenchmark behind tools/ab_gemm.py / tools/bench_gemm.py, and czc_test_set_option flips process-wide kernel-family
 * switches for A/B runs.  The product library (include/conzic_hip.h) exports none of these; this library reaches its
 * launchers and switches through czc_internal_hooks, links against nothing but its C ABI, and is loaded next to it by tests and tools only (conzic_amd/native.py: load_test()).
 */
#ifndef CONZIC_HIP_TEST_H
#define CONZIC_HIP_TEST_H

#include "conzic_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* C[M,N] = A[M,K] * W[N,K]^T (+bias) (+activation: 0 none, 1 quick_gelu, 2 gelu_erf) (+resid[M,N]).
 * act | 0x100: take the result through the activation-typed output path (bf16 / split-fp16 / f32 per
 * `precision`, resid must be NULL) instead of the fp32 one -- the path the tower-internal layers use. */
int czc_test_gemm(int precision, int M, int N, int K, const float* A, const float* W, const float* bias,
                  const float* resid, int act, float* C);
/* Residual-add layer on a 2-byte residual stream (the bf16 engine's CLIP-text tower, csrc/kernels.h GemmArgs::x16):
 * x_out[M,N] = fp16(fp16(resid) + A[M,K] * W[N,K]^T + bias), the sum formed in fp32; returned as fp32.  N, K % 8 == 0. */
int czc_test_gemm_x16(int precision, int M, int N, int K, const float* A, const float* W, const float* bias, const float* resid,
                      float* x_out, float* part_out /* NULL or [N/32][M][2]: (sum, sum of squares) per row and 32-column block */);
/* LayerNorm folded into the K = 512 GEMM: out[M,N] = act(LN(fp16(x); gamma, beta, eps) . W^T + bias), from x itself, the folded
 * (gain applied, rows centred) fp16 weights and the row statistics derived from `part` [16][M][2] (partials of fp16(x) as a
 * producer GEMM writes them).  rowsum_out: NULL or [N], what is left of the sum of each stored weight row. */
int czc_test_ln_fold_gemm(int precision, int M, int N, const float* x, const float* W, const float* gamma, const float* beta,
                          const float* bias, const float* part, float eps, int act, float* out, float* rowsum_out);
/* LayerNorm of fp16 rows, 512 wide: y[M,512] = LN(fp16(x)) rounded to the operand type of `precision` (bf16 / fp16). */
int czc_test_layernorm_x16(int precision, int M, const float* x, const float* gamma, const float* beta, float eps, float* y);

/* Full-row GEMM with the following LayerNorm in its epilogue (bf16 / fp16 operands, 512 columns, K % 32 == 0):
 *   x_out[M,512] = resid + A[M,K] * W[512,K]^T + bias;  y_out = LayerNorm(x_out; gamma, beta, eps) in the operand type */
int czc_test_gemm_rowln(int precision, int M, int K, const float* A, const float* W, const float* bias, const float* resid,
                        const float* gamma, const float* beta, float eps, float* x_out, float* y_out);
/* GEMM microbenchmark on device-resident data: ms per launch (tools/bench_gemm.py); use256: 0 128x128 kernel,
 * 1 the default choice among the 256x256 LDS-DMA ring kernels, 3 the loader-wave ring kernel, 7 the ping-pong ring
 * kernel, 6 the weight-stationary kernel where eligible. */
int czc_bench_gemm(int precision, int M, int N, int K, int act, int out_mode, int iters, int use256, double* ms_out);
/* Process-wide kernel-family switches for tests and tools: "gemm256" 0|1|3|5, "wreg" 0|1, "gemm256s" 0|1, "skinny",
 * "splitk", "gemm_deep" 0|1|2, "gemm_small_tiles", "mfma_attention", "attention_image" 0|1|2 (2 = force), the "*_min_m"
 * row-count thresholds, "wreg_stats_in_kernel", "bridge_no_table" (czc_test_bridge, czc_test_bridge_cand), "bench_pad" (row padding of
 * czc_bench_gemm operands).  Any other name fails with CZC_ERR_ARG. */
int czc_test_set_option(const char* name, int value);
int czc_test_layernorm(int precision, int M, int H, const float* x, const float* gamma, const float* beta, float eps,
                       float* y);
/* qkv [sum(len), 3*heads*64] packed sequences; causal 0/1; scale; out [sum(len), heads*64] */
int czc_test_attention(int precision, int n_seq, const int32_t* seq_len, int heads, int causal, float scale,
                       const float* qkv, float* out);
/* One attention launch on a host-given SHARED-PREFIX plan, laid out as the engine lays it out: B trunk segments (trunk_len[B]
 * rows, no prefix), then the B*K branch segments back to back (own_len[B*K] rows; branch (b,k) sees the trunk of image b as
 * key/value-only prefix and its own rows causally); own_off = exclusive scan, max_own / max_keys / the per-image maxima
 * computed as the engine computes them (pass_img_max 0: SegTable::img_max is null).
 *   kernel 0: launch_attention with the prefix tables (attention_mfma_kernel / attention_mfma_split_kernel /
 *             attention_valu_kernel, whichever `precision` and the "mfma_attention" switch select);
 *          1: launch_attention_shared / _split with the per-group kernels (attention_branch_kernel / _split_kernel);
 *          2: launch_attention_shared with attention_image_kernel forced (bf16 / fp16; the launcher still falls back to the
 *             per-group kernel where the per-image one cannot serve the plan).
 *   precision: 1 f32 (kernel 0 only), 0 bf16, 4 fp16, 3 split-fp16 (kernels 0, 1).  The "attention_image" switch is set for the
 *   call and restored.
 * qkv: fp32 [rows, 3*heads*64] (rows = sum of all lengths), rounded to the operand type on the device.
 * out: fp32 [CZC_TEST_PLAN_GUARD + rows + CZC_TEST_PLAN_GUARD, heads*64]: the device output buffer WITH the guard rows the
 *   hook keeps in front of and behind the plan rows inside its own allocations.  The output is pre-filled with bytes 0x5a (so
 *   an unwritten element reads back as that pattern in the output type) and the guard rows of the device qkv hold NaNs of the
 *   operand type: a stray read or write shows in the result, and stays inside the hook's buffers.
 * Returns 0, CZC_TEST_REFUSED (not an error: the packed launcher returned -1 for this plan, nothing was launched, `out` is
 * the untouched pattern) or a CZC_ERR_* status. */
#define CZC_TEST_REFUSED 100
#define CZC_TEST_PLAN_GUARD 32
int czc_test_attention_plan(int precision, int kernel, int B, int K, int heads, float scale, const int32_t* trunk_len,
                            const int32_t* own_len, int pass_img_max, const float* qkv, float* out);
/* One launch_attention call on PLAIN segments (no prefix) in the forms the BERT and vision towers pass them, through
 * attention_mfma_kernel / attention_mfma_split_kernel / attention_valu_kernel, whichever `precision` (1 f32, 0 bf16, 4 fp16,
 * 3 split-fp16) and the "mfma_attention" switch select:
 *   seq_len [n_seg]: own_off / own_len tables, rows back to back (own_off = exclusive scan), prefix tables null; a segment may
 *     have 0 rows.  seq_len NULL: the fixed_T form, SegTable{NULL, NULL, NULL, NULL, n_seg, fixed_T} (fixed_T is ignored otherwise).
 *   max_keys: what the launcher sizes the kernels' shared memory with; 0 = the longest segment.  A value below the longest
 *     segment is refused here with CZC_ERR_ARG (the kernels trust it); one the launcher does not serve (outside 1..96) comes back
 *     as the launcher's error.  n_seg 0 is an empty launch: it succeeds and writes nothing.
 *   causal 0 | 1.  qkv: fp32 [rows, 3*heads*64] (rows = sum of the lengths), rounded to the operand type on the device.
 *   out: fp32 [CZC_TEST_PLAN_GUARD + rows + CZC_TEST_PLAN_GUARD, heads*64], guarded and pre-filled as czc_test_attention_plan's
 *     (NaN rows of the operand type around qkv, bytes 0x5a in every byte of the device output before the launch).
 * Returns 0 or a CZC_ERR_* status. */
int czc_test_attention_seq(int precision, int n_seg, const int32_t* seq_len, int fixed_T, int max_keys, int heads, int causal,
                           float scale, const float* qkv, float* out);
/* attention_image_kernel's POOLED mode (launch_attention_image_pooled: the tower's last layer) on the same kind of host-given
 * plan, per-image kernel forced, precision 0 bf16 / 4 fp16:
 *   qkv  fp32 [rows, 3*heads*64]: k / v of all packed rows (its q columns must not be read: the caller may poison them);
 *   qc   fp32 [B*K, heads*64]: one q row per candidate;   rep [B*K]: the plan's de-duplication table (candidate i of image b
 *        rides on candidate rep[i] of that image, its own index where it has rows) -- a candidate with own_len 0 receives the
 *        compact row of its representative;
 *   out  fp32 [CZC_TEST_PLAN_GUARD + B*K + CZC_TEST_PLAN_GUARD, heads*64]: the compact context rows with their guard rows.
 * Guards and pre-fills as czc_test_attention_plan (NaN rows around qkv and qc, bytes 0x5a in out).  Returns 0 or a CZC_ERR_*
 * status (a plan the per-image kernel does not serve is an error here). */
int czc_test_attention_pooled(int precision, int B, int K, int heads, float scale, const int32_t* trunk_len, const int32_t* own_len,
                              const int32_t* rep, const float* qkv, const float* qc, float* out);
/* attention_image_kernel's MAPPED mode (launch_attention_shared_mapped: the tower's layer 0 on distinct rows) on such a plan,
 * per-image kernel forced, precision 0 bf16 / 4 fp16: qkv fp32 [n_rows, 3*heads*64] holds packed row r of the plan at row
 * rowmap[r] (rowmap [rows]; trunk rows must map to themselves), out as czc_test_attention_plan's (packed context rows with
 * guard rows, pre-filled with bytes 0x5a); NaN rows around the n_rows rows of qkv. */
int czc_test_attention_mapped(int precision, int B, int K, int heads, float scale, const int32_t* trunk_len, const int32_t* own_len,
                              const int32_t* rowmap, int n_rows, const float* qkv, float* out);
/* The engine's plan chain with the layer-0 distinct-row plan (launch_prefix_plan with sharing -> launch_layer0_count ->
 * launch_scan -> launch_prefix_finish [-> launch_layer0_map when M > 0 and n_dist > 0: the sizes a first call returned]) on
 * clip_ids [B*K, 77] / clip_len [B*K].  Outputs, each with CZC_TEST_GUARD words around it (see below): own_off [S + 1],
 * own_len [S] (S = B + B*K), dcount [B], totals [12] ([0] rows, [6] trunk rows, [8] distinct branch rows), rowmap [max(M, 1)],
 * dist [max(n_dist, 1)]. */
int czc_test_layer0_plan(int B, int K, const int32_t* clip_ids, const int32_t* clip_len, int dedup, int32_t* own_off, int32_t* own_len,
                         int32_t* dcount, int32_t* totals, int M, int32_t* rowmap, int n_dist, int32_t* dist);
/* The text tower of `engine` (a czc_engine*) on host-given CLIP id rows clip_ids [B*K, 77] / clip_len [B*K] of B images x K
 * candidates, through the step's own plan and tower (shared prefix, de-duplication and every other option as the engine holds
 * them): feat fp32 [B*K, clip_proj], *n_dup = candidates that ride on an identical one of their image. */
int czc_test_text_tower(void* engine, int B, int K, const int32_t* clip_ids, const int32_t* clip_len, float* feat, int32_t* n_dup);
int czc_test_topk(int B, int V, int K, const float* logits, const float* mask, float temperature, int dot_id,
                  int dot_allowed, float* probs, int32_t* idxs, int32_t* cand);
int czc_test_bridge(const czc_bridge_tables* t, const czc_config* cfg, int n_rows, int T, const int32_t* rows,
                    int32_t* clip_ids, int32_t* clip_len);
int czc_test_combine(int B, int K, int D, const float* text_feat, const float* img_embeds, float logit_scale,
                     const float* probs, const float* senti_raw, const float* repeats, const czc_hyper* hp,
                     float* clip_score, float* clip_ref, float* final_score, int32_t* best);
/* czc_test_combine through the drawing instantiation of the combine kernel: draw [B] (a tau == 0 row keeps the first argmax),
 * step = the step index added to every record's step0. */
int czc_test_combine_draw(int B, int K, int D, const float* text_feat, const float* img_embeds, float logit_scale,
                          const float* probs, const float* senti_raw, const float* repeats, const czc_hyper* hp,
                          const czc_draw* draw, uint32_t step, float* final_score, int32_t* best);

/* ---- the integer and selection side of the screen-then-refine engine (csrc/combine.hip, csrc/bridge.hip), one launcher chain
 * at a time, with the buffer preparation of the engine (tests/refine_ref.py states each operation in numpy).
 * EVERY OUTPUT ARRAY below holds CZC_TEST_GUARD + n + CZC_TEST_GUARD 4-byte words for the n the comment names: the device
 * buffer sits inside a larger allocation pre-filled with bytes 0x5a and comes back whole, so a stray store shows in the guard
 * words and a word the kernels do not write reads back as the pattern. */
#define CZC_TEST_GUARD 64
/* launch_scan: off [n + 1] = exclusive scan of len [n], totals [2] = (sum, max) */
int czc_test_scan(int n, const int32_t* len, int32_t* off, int32_t* totals);
/* launch_prefix_plan -> launch_scan -> launch_prefix_finish on clip_ids [B*K, 77] / clip_len [B*K], S = B + B*K segment slots:
 * own_len, pre_len, seg_src, seg_pos0, pre_off [S]; own_off [S + 1]; eos_idx, rep [B*K] (rep only with dedup); img_max [B];
 * totals [8], zeroed first: [0] rows, [1] longest segment, [3] longest sequence, [4] longest branch, [5] duplicates, [6] trunk
 * rows, [7] causal (query, key) pairs. */
int czc_test_prefix_plan(int B, int K, int share, int dedup, const int32_t* clip_ids, const int32_t* clip_len, int32_t* own_len,
                         int32_t* pre_len, int32_t* seg_src, int32_t* seg_pos0, int32_t* own_off, int32_t* pre_off, int32_t* eos_idx,
                         int32_t* rep, int32_t* img_max, int32_t* totals);
/* form 0 launch_refine_select (theta, beta), 1 launch_refine_select_rows (theta_base, scale, hyper [B]), 2
 * launch_refine_select_draw (draw [B]; hyper [B] or NULL = the scalar theta / beta) on clip_score / final_score [B, K]:
 * gated [2] (zeroed first), kind, list [B*K], count [B]. */
int czc_test_refine_select(int form, int B, int K, const float* clip_score, const float* final_score, float theta, float theta_base,
                           float scale, int m_samples, float gate_h, float beta, int need_cos, const czc_hyper* hyper,
                           const czc_draw* draw, int32_t* gated, int32_t* kind, int32_t* list, int32_t* count);
/* the refine pass's plan: launch_scan(count) -> launch_refine_plan -> launch_scan(own_len) -> launch_refine_finish, own_len and
 * the totals zeroed first.  clip_len, list [B*K], trunk_len, count [B] -> count_off [B + 1]; own_len, pre_len, seg_src, seg_pos0,
 * pre_off [S]; own_off [S + 1]; rlist, eos_idx [B*K]; img_max [B]; totals [16]: [0] rows, [1] longest segment, [3] longest
 * sequence, [4] longest branch, [7] pairs, [8] R, [9] Kr. */
int czc_test_refine_plan(int B, int K, const int32_t* clip_len, const int32_t* trunk_len, const int32_t* list, const int32_t* count,
                         int32_t* count_off, int32_t* own_len, int32_t* pre_len, int32_t* seg_src, int32_t* seg_pos0, int32_t* own_off,
                         int32_t* pre_off, int32_t* rlist, int32_t* eos_idx, int32_t* img_max, int32_t* totals);
/* launch_refine_cosine: text_feat [n_rows_max, D] of which the first n_rows count, img_embeds [B, D] (L2-normalised on the
 * device), rlist [n_rows_max] -> cos_out [B*K], nonfinite [8] (zeroed first). */
int czc_test_refine_cosine(int n_rows_max, int n_rows, int B, int K, int D, const float* text_feat, const float* img_embeds,
                           const int32_t* rlist, float* cos_out, int32_t* nonfinite);
/* launch_combine with refine_kind / refine_cos [B, K]: cos_in [B, K] enters through clip_ref (no text features) ->
 * clip_score, clip_ref, final_score [B*K], best, best_cos [B], nonfinite [8] (zeroed first). */
int czc_test_combine_refine(int B, int K, float logit_scale, const float* cos_in, const float* probs, const czc_hyper* hp,
                            const int32_t* refine_kind, const float* refine_cos, float refine_guard, float* clip_score, float* clip_ref,
                            float* final_score, int32_t* best, float* best_cos, int32_t* nonfinite);
/* launch_combine through the rival instantiation (czc_generate_rows_vs): B rows with own image image_of_row[b] of img_all
 * [n_img, D] (L2-normalised on the device; the rows' own embeddings are the gathered copy), rival_idx [B, M] into img_all (-1 =
 * empty, filled slots first), delta [B], hp [B] (control 0), draw [B] or NULL = no row draws, step as in czc_test_combine_draw ->
 * clip_ref, disc, final_score [B*K], best [B], nonfinite [8] (zeroed first); guarded outputs as above. */
int czc_test_combine_rivals(int B, int K, int D, const float* text_feat, const float* img_all, int n_img, const int32_t* image_of_row,
                            const int32_t* rival_idx, int M, const float* delta, float logit_scale, const float* probs,
                            const czc_hyper* hp, const czc_draw* draw, uint32_t step, float* clip_ref, float* disc, float* final_score,
                            int32_t* best, int32_t* nonfinite);
/* launch_combine in every instantiation without rivals, on B rows of K candidates (tests/combine_ref.py states the operation):
 *   form 0 the scalar form (write-back column gen_idx), 1 per-row columns (gen_rows [B]), 2 per-row columns and hyper-parameters
 *   (hp [B]), 3 those and the draw (draw [B], draw_step as in czc_test_combine_draw).  Forms 0 and 1 read ONE record of hp; draw is
 *   NULL unless form 3; gen_rows NULL (forms 1-3, inp NULL) = zeros.
 *   Cosines: text_feat [B*K, D] and img_embeds [B, D] (L2-normalised on the device), cos_in NULL -- or text_feat NULL and cos_in
 *   [B*K], which is placed in clip_ref before the launch (the form the refine engine's second combine uses).
 *   probs [B*K], cand [B*K] (the ids written back), senti_raw / repeats [B*K] or NULL.
 *   inp_in [B*T] or NULL = nothing is written back; inp_out [B*T] receives the rows after the launch (both or neither).
 *   run [B] or NULL (forms 2, 3): hp / draw hold R full records, the B rows' records are gathered on the device by
 *   launch_gather_row_hyper / launch_gather_row_draw (record of row i = record run[i]) and come back as stored in hp_out [B*6 words]
 *   / draw_out [B*4 words].
 * Outputs (guarded as above): clip_score, clip_ref, final_score [B*K]; best, best_cos [B]; nonfinite [8] (zeroed first); inp_out.
 * scale_out (one plain float, or NULL): expf(logit_scale) as the kernel is handed it.
 * Checked here first (CZC_ERR_ARG): every write-back column in [0, T), every run entry in [0, R), a control-1 row has senti_raw
 * and repeats, a control-2 row has senti_raw.  K beyond the launcher's limit: CZC_TEST_REFUSED -- launch_combine launched neither
 * the cosine kernel nor the combine kernel (the hook's own preparation, launch_l2_normalize and the record gathers into its scratch,
 * has run) and every output is the untouched pattern (clip_ref: cos_in where that was given, inp_out: inp_in). */
int czc_test_combine_rows(int B, int K, int D, int T, const float* text_feat, const float* img_embeds, const float* cos_in,
                          float logit_scale, const float* probs, const int32_t* cand, const float* senti_raw, const float* repeats,
                          int form, const czc_hyper* hp, const czc_draw* draw, uint32_t draw_step, int gen_idx, const int32_t* gen_rows,
                          const int32_t* run, int R, const int32_t* inp_in, int32_t* inp_out, float* clip_score, float* clip_ref,
                          float* final_score, int32_t* best, float* best_cos, int32_t* nonfinite, int32_t* hp_out, int32_t* draw_out,
                          float* scale_out);

/* ---- the row, embedding, mover and memo kernels one by one (csrc/rowops.hip, ragged.hip, memo.hip, memo_rows.hip; numpy models in
 * tests/rowops_ref.py and tests/memo_ref.py).  EVERY OUTPUT ARRAY holds CZC_TEST_GUARD + n + CZC_TEST_GUARD 4-byte words as above and
 * comes back RAW: an activation-typed output of n elements is the bytes the kernel stored, in (n * element size + 3) / 4 words (bf16 /
 * fp16: 2-byte elements; split-fp16: groups of 8 elements as 16 bytes of hi parts, then 16 bytes of lo parts; f32: the floats), so
 * results can be compared bit for bit.  Every index a kernel follows is checked on the host first (CZC_ERR_ARG).  A launcher that
 * refuses its shape launches nothing: the call returns CZC_TEST_REFUSED and every output holds the untouched pattern. */
/* launch_layernorm on x [n_src, H]: row m reads row row_idx[m] (NULL: m).  mode: 1 typed output y_act, 2 fp32 output y_f32, 4 the
 * in-place form (y_f32 is x itself; needs 2, no row_idx, n_src == M; y_f32 then returns the x buffer). */
int czc_test_layernorm_rows(int precision, int M, int H, int n_src, const float* x, const int32_t* row_idx, const float* gamma,
                            const float* beta, float eps, int mode, int32_t* y_act, float* y_f32);
/* launch_layernorm_x16 on fp16(x) [n_src, H] with row_idx (H = 512 is the only width it serves) -> y_act [M, H] 2-byte elements */
int czc_test_layernorm_x16_rows(int precision, int M, int H, int n_src, const float* x, const int32_t* row_idx, const float* gamma,
                                const float* beta, float eps, int32_t* y_act);
/* launch_layernorm_splitk: slabs [nslab, M, ld], bias [H] or NULL, resid [M, ldr] or NULL -> y_act, y_f32 [M, H] */
int czc_test_layernorm_splitk(int precision, int nslab, int M, int H, int ld, const float* slabs, const float* bias, const float* resid,
                              int ldr, const float* gamma, const float* beta, float eps, int32_t* y_act, float* y_f32);
/* launch_ln_finalize: part [nblk, ld, 2] (sum, sum of squares per 32-column block) -> stat [M, 2] (mean, rstd) */
int czc_test_ln_finalize(int nblk, int M, int ld, const float* part, float eps, float* stat);
/* launch_bert_embed: ids [B, T] < V, word [V, H], pos [n_pos, H], type0 [H] -> y_act, y_f32 [B*T, H] */
int czc_test_bert_embed(int precision, int B, int T, int H, int V, int n_pos, const int32_t* ids, const float* word, const float* pos,
                        const float* type0, const float* gamma, const float* beta, float eps, int32_t* y_act, float* y_f32);
/* launch_bert_embed_ragged: ids [n_id_rows, ids_stride], run [n] or NULL, row_off [n + 1], row_len [n] -> y_act, y_f32 [n_out_rows, H] */
int czc_test_bert_embed_ragged(int precision, int n, int n_id_rows, int ids_stride, int max_T, int H, int V, int n_pos, const int32_t* ids,
                               const int32_t* run, const int32_t* row_off, const int32_t* row_len, int n_out_rows, const float* word,
                               const float* pos, const float* type0, const float* gamma, const float* beta, float eps, int32_t* y_act,
                               float* y_f32);
/* launch_clip_embed on a host-given segment plan; mode 0 fp32 rows, 1 fp16 rows, 2 fp16 rows + stat [n_out_rows, 2] (mean, rstd of the
 * stored row) -> x_out [n_out_rows, H] (4- or 2-byte elements) */
int czc_test_clip_embed(int mode, int n_seg, int max_len, int H, int n_id_rows, int ids_stride, const int32_t* ids, const int32_t* seg_src,
                        const int32_t* seg_pos0, const int32_t* own_off, const int32_t* own_len, int V, int n_pos, const float* tok,
                        const float* pos, int n_out_rows, float eps, int32_t* x_out, float* stat);
/* launch_im2col: pixels [B, 3, S, S] -> out [B * (S/p)^2, 3*p*p] typed */
int czc_test_im2col(int precision, int B, int S, int p, const float* pixels, int32_t* out);
/* launch_vision_assemble: patch_out [B*P, H], cls [H], pos [P + 1, H] -> x [B, P + 1, H] */
int czc_test_vision_assemble(int B, int P, int H, const float* patch_out, const float* cls, const float* pos, float* x);
/* launch_l2_normalize: x [M, D] -> y [M, D] */
int czc_test_l2_normalize(int M, int D, const float* x, float* y);
/* dst[m] = src[idx[m]]; kind 0 launch_gather_rows_f32 (W floats per row), 1 launch_gather_rows_bytes (W bytes per row, W % 4 == 0),
 * 2 launch_gather_rows_w32 (W words per row); src n_src rows, dst M rows */
int czc_test_gather_rows(int kind, int M, int W, int n_src, const int32_t* src, const int32_t* idx, int32_t* dst);
/* gen_rows NULL: launch_mask_positions at gen_idx, else launch_mask_positions_rows; inp [B, T] -> inp_out */
int czc_test_mask_positions(int B, int T, int gen_idx, const int32_t* gen_rows, int n_mask, int mask_id, const int32_t* inp, int32_t* inp_out);
/* launch_tie_rows: inp [R, T], col, grp_of_row [R], grp_off [G + 1], grp_rows [grp_off[G]] -> inp_out */
int czc_test_tie_rows(int R, int T, int G, const int32_t* inp, const int32_t* col, const int32_t* grp_of_row, const int32_t* grp_off,
                      const int32_t* grp_rows, int32_t* inp_out);
/* The image memo for one sub-step, chained as the engine chains it: launch_memo_check; with stages != 0 and n = tot[0] read back:
 * launch_memo_fill when n < B; when n > 0 launch_memo_gather (use_list: the compact batch of the listed images, else the whole batch in
 * place), the step (compact row i takes new_rows / new_cos / new_max of its image), launch_memo_scatter.  record 0: no key and no entry
 * is written.  In: inp, key, new_rows, ent_rows [B, T]; img_max [2, B]; img_n [B, D]; new_cos, new_max, ent_cos, ent_max, bcos_in [B].
 * Out: hit, list [B]; tot [4]; key_out, inp_out, ent_rows_out, inp_c [B, T]; bcos_out, ent_cos_out, ent_max_out [B]; img_c [B, D]. */
int czc_test_memo_chain(int B, int T, int D, int gen_idx, int n_mask, int mask_id, int n_sub, int stages, int use_list, int record,
                        const int32_t* inp, const int32_t* key, const int32_t* img_max, const float* img_n, const int32_t* new_rows,
                        const float* new_cos, const int32_t* new_max, const int32_t* ent_rows, const float* ent_cos, const int32_t* ent_max,
                        const float* bcos_in, int32_t* hit, int32_t* list, int32_t* tot, int32_t* key_out, int32_t* inp_out, float* bcos_out,
                        int32_t* ent_rows_out, float* ent_cos_out, int32_t* ent_max_out, int32_t* inp_c, float* img_c);
/* The rows memo for sub-step j of a group, chained likewise: launch_memo_rows_check; with stages != 0: launch_memo_rows_fill when n < R;
 * when n > 0 launch_memo_rows_gather (use_list: compact batch, else all rows in place and recording only), the step,
 * launch_memo_rows_scatter.  Table in / out: valid, sig [L, R]; key [L, R, T]; rows [L, 2, R, T]; cos, imax [L, 2, R].  col0, col1 (NULL:
 * one-step group), col, dot [R]; tau NULL or [R].  Out: hit, list, col_c, dot_c, bcos_out [R]; cnt [(R + 255) / 256]; tot [4]; inp_out,
 * inp_c [R, T]; img_c [R, D]. */
int czc_test_memo_rows_chain(int R, int T, int L, int seed_len, int D, int n_mask0, int n_sub, int mask_id, int j, int stages, int use_list,
                             int record, const int32_t* inp, const int32_t* col0, const int32_t* col1, const float* tau, const int32_t* col,
                             const int32_t* dot, const float* img_n, const int32_t* new_rows, const float* new_cos, const int32_t* new_max,
                             const float* bcos_in, const int32_t* valid, const int32_t* sig, const int32_t* key, const int32_t* rows,
                             const float* cos, const int32_t* imax, int32_t* valid_out, int32_t* sig_out, int32_t* key_out, int32_t* rows_out,
                             float* cos_out, int32_t* imax_out, int32_t* hit, int32_t* cnt, int32_t* list, int32_t* tot, int32_t* inp_out,
                             float* bcos_out, int32_t* inp_c, float* img_c, int32_t* col_c, int32_t* dot_c);

/* ---- caption fluency (csrc/fluency.hip; numpy models in tests/fluency_ref.py).  Plain output arrays of the sizes named. */
/* launch_logprob_target on logits [N, V], target [N] (checked: inside [0, V)) -> logp, rank [N]; nonfinite [1] (zeroed first).  The
 * device logits keep the row stride V, so odd V give rows that do not start on a 16-byte boundary. */
int czc_test_logprob(int N, int V, const float* logits, const int32_t* target, float temperature, float* logp, int32_t* rank,
                     int32_t* nonfinite);
/* The expansion of czc_fluency_rows: the host tables (fluency_expand_tables) and launch_expand_mask_rows on rows [R, T] with
 * len_of_row [R] (NULL: every row has T - seed_len - 1 words) -> *n_seq = N = sum L_r, ids_out [N, T], target, gen_rows [N]
 * (the caller sizes them for N). */
int czc_test_expand_mask(int R, int T, int seed_len, int mask_id, const int32_t* rows, const int32_t* len_of_row, int32_t* ids_out,
                         int32_t* target, int32_t* gen_rows, int32_t* n_seq);

/* ---- the text bridge with candidates and the per-row forms of the top-K selection (csrc/bridge.hip, csrc/topk.hip; string-level
 * reference in tests/bridge_ref.py).  EVERY OUTPUT ARRAY holds CZC_TEST_GUARD + n + CZC_TEST_GUARD 4-byte words, pre-filled with bytes
 * 0x5a, and comes back raw.  A launcher's own refusal returns CZC_TEST_REFUSED with every output untouched. */
/* bridge_kernel on inp [B, T] with column gen of row b replaced by cand [B, K] (one thread per candidate row):
 *   form 0 launch_bridge (gen_idx; gen_rows, row_len, hp_rows are not passed on), 1 launch_bridge_rows (gen_rows [B], row_len [B] or
 *   NULL, the scalar `negative`), 2 launch_bridge_rows_hp (hp_rows [B]: control / negative per row).
 * Control tables, each may be NULL: lexicon [V]; lex_pos [V, 5] with lex_cls [V]; tag_of_token [V] with masks [n_masks].
 * The bridge tables are uploaded, hashed and tabulated as czc_test_bridge does ("bridge_no_table" applies).  Checked on the host
 * (CZC_ERR_ARG): every id of inp and cand inside the vocabulary, every gen inside the row, 1 <= row_len <= T <= CZC_MAX_BERT_LEN,
 * lex_cls < 5, tags < 15.
 * -> clip_ids [B*K, 77], clip_len, senti_raw, repeats [B*K], overflow [1] (zeroed first: the number of candidate rows that took the
 * kernel's overflow path -- data, not an error status). */
int czc_test_bridge_cand(const czc_bridge_tables* t, int form, int B, int T, int K, const int32_t* inp, int gen_idx, const int32_t* gen_rows,
                         const int32_t* row_len, const int32_t* cand, const float* lexicon, const float* lex_pos, const uint8_t* lex_cls,
                         const uint8_t* tag_of_token, const uint16_t* masks, int n_masks, int negative, const czc_hyper* hp_rows,
                         int32_t* clip_ids, int32_t* clip_len, float* senti_raw, float* repeats, int32_t* overflow);
/* softmax_mask_topk_kernel in its per-row forms on logits [B, V], mask [V]: form 1 launch_softmax_mask_topk_rows (temperature,
 * dot_rows [B]), 2 launch_softmax_mask_topk_rows_hp (hp_rows [B]: the row's temperature; dot_rows [B]) -> probs, idxs, cand [B*K]. */
int czc_test_topk_rows(int form, int B, int V, int K, const float* logits, const float* mask, float temperature, int dot_id,
                       const int32_t* dot_rows, const czc_hyper* hp_rows, float* probs, int32_t* idxs, int32_t* cand);
/* The same kernel with a vocabulary set per row (launch_softmax_mask_topk_rows_vocab, czc_generate_rows_vocab): set_rows [B] in
 * [-1, n_sets) picks one of the bitsets bits [n_sets, W], W = ceil(V / 32); hp_rows [B] and dot_rows [B] as in form 2.  Checked on
 * the host (CZC_ERR_ARG): every set index.  A null hp_rows, dot_rows, set_rows or bits, or a W other than ceil(V / 32), is the
 * launcher's own refusal (CZC_TEST_REFUSED). */
int czc_test_topk_rows_vocab(int B, int V, int K, const float* logits, const float* mask, int dot_id, const int32_t* dot_rows,
                             const czc_hyper* hp_rows, const int32_t* set_rows, const uint32_t* bits, int n_sets, int W, float* probs,
                             int32_t* idxs, int32_t* cand);

/* ---- every GEMM family on strided, windowed and in-place buffers (csrc/gemm.hip, gemm256.hip, gemm_wreg.hip; host reference and
 * checker in tests/gemm_layout.py).  The kernel family a launch went to is recorded by the launcher (csrc/kernels.h GemmFamily): */
#define CZC_GEMM_FAMILY_NONE 0 /* nothing launched */
#define CZC_GEMM_FAMILY_TILED_VEC 1
#define CZC_GEMM_FAMILY_TILED_SCALAR 2
#define CZC_GEMM_FAMILY_SPLITK 3
#define CZC_GEMM_FAMILY_SKINNY 4
#define CZC_GEMM_FAMILY_RING_LOADER 5
#define CZC_GEMM_FAMILY_RING_PINGPONG 6
#define CZC_GEMM_FAMILY_RING_SPLIT 7
#define CZC_GEMM_FAMILY_WREG 8
#define CZC_GEMM_FAMILY_WREG_LNF 9
#define CZC_GEMM_FAMILY_WREG_RESID 10
#define CZC_GEMM_FAMILY_ROWLN 11
/* the family of the calling thread's last czc_test_gemm* / czc_bench_gemm launch */
int czc_test_gemm_family(void);

#define CZC_GEMM_FORM_PLAIN 0 /* launch_gemm: out_f32 (default), out_act (TYPED_OUT) or both (BOTH_OUTPUTS) */
#define CZC_GEMM_FORM_X16 1   /* launch_gemm on the 2-byte residual stream: resid / out_f32 are fp16 rows; optional row_part */
#define CZC_GEMM_FORM_LNF 2   /* folded LayerNorm, prepared exactly as czc_test_ln_fold_gemm prepares it (K = 512, out_act) */
#define CZC_GEMM_FORM_ROWLN 3 /* launch_gemm_rowln (N = ldc = 512): out_f32 = x and out_act = LayerNorm(x) */
#define CZC_GEMM_IN_PLACE 1     /* resid and out_f32 are ONE buffer (ldr == ldc) */
#define CZC_GEMM_BOTH_OUTPUTS 2 /* plain form: out_f32 and out_act from one launch */
#define CZC_GEMM_TYPED_OUT 4    /* plain form: out_act only */
#define CZC_TEST_LAYOUT_GUARD 8 /* guard rows in front of every 2-D buffer of the hook */
/* One GEMM launch whose every leading dimension, output window and aliasing the caller chooses.  Host inputs are DENSE fp32
 * arrays; the hook rounds them to the operand type on the device and places them in its own padded buffers:
 *   rows r of a [rows, width] array sit at elements (CZC_TEST_LAYOUT_GUARD + r) * ld + c0 .. + width of a buffer of
 *   CZC_TEST_LAYOUT_GUARD + rows + back(rows) rows of ld elements, back(rows) = (256 - rows % 256) % 256 + CZC_TEST_LAYOUT_GUARD
 *   (the guard behind the rows reaches past the end of the last 256-row tile).
 * A [M, K] at lda, W [N, K] at ldw and a residual that has a buffer of its own ([M, N] at ldr, c0 columns into its rows) are
 * OPERANDS: every pad column and guard row holds the quiet-NaN pattern of the element type.  out_f32 and out_act are OUTPUTS
 * ([M, N] at ldc, c0 columns into their rows): every byte pre-filled with 0x5a, and the WHOLE buffer (guards, pads, window) comes
 * back raw in its element type (out_f32: fp32, or fp16 in the x16 form; out_act: the operand type of `precision`), bytes()
 * = rows_total * ldc * element size.  IN_PLACE: the residual is written into the output buffer's owned elements instead (the
 * rest of that buffer keeps the 0x5a pattern).  bias [N] is passed as it stands (the caller windows W and bias by choosing them).
 *   x16: part_ld > 0 asks for row_part [N / 32][part_ld] float2; part_out receives CZC_TEST_GUARD + N / 32 * part_ld * 2 +
 *        CZC_TEST_GUARD words, 0x5a-filled first.
 *   lnf: A = x (fp16 rows), W / bias / gamma / beta fp32 folded by fold_ln_kernel, statistics from ln_part [16][M][2] through
 *        ln_finalize_kernel, or inside the GEMM where gemm_wreg_stats_in_kernel(M, N) allows (option "wreg_stats_in_kernel").
 *   rowln: gamma / beta [512]; the caller sets "rowln_min_m".
 * Which kernel serves the launch follows the shape and the czc_test_set_option switches, as in the product.
 * Returns the CZC_GEMM_FAMILY_* that served the launch (> 0), 0 when the launcher refused it (nothing ran, every output is the
 * untouched pattern, the calling thread's last-error text says why), or -CZC_ERR_* for a failure of the hook itself. */
typedef struct czc_gemm_layout {
  int32_t precision, form, M, N, K, act;
  int32_t lda, ldw, ldc, ldr;
  int32_t c0, flags, part_ld;
  float eps;
  const float *A, *W, *bias, *resid, *gamma, *beta, *ln_part;
  void *out_f32, *out_act;
  float* part_out;
} czc_gemm_layout;
int czc_test_gemm_layout(const czc_gemm_layout* c);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CONZIC_HIP_TEST_H */
