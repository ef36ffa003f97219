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
 * row-count thresholds, "wreg_stats_in_kernel", "bridge_no_table" (czc_test_bridge), "bench_pad" (row padding of
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

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CONZIC_HIP_TEST_H */
