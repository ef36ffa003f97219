// Host-side launchers of the gfx950 kernels (one translation unit per kernel family).
#pragma once
#include <vector>

#include "common.h"

namespace czc {

// ---- gemm.hip ---------------------------------------------------------------------------
// C[M,N] = A[M,K] . W[N,K]^T  (+bias[N]) (act) (+resid[M,N] fp32)
// A, W are row-major with K contiguous (nn.Linear layout), element type by `prec`
// (bf16_t or float).  out_act (same element type, may be null) and/or out_f32 (may be null)
// are written with leading dimension ldc.  resid may alias out_f32.
struct GemmArgs {
  const void* A = nullptr; int lda = 0;
  const void* W = nullptr; int ldw = 0;
  const float* bias = nullptr;
  const float* resid = nullptr; int ldr = 0;
  void* out_act = nullptr; float* out_f32 = nullptr; int ldc = 0;
  int M = 0, N = 0, K = 0;
  int act = 0;
  int f16 = 0;  // 2-byte operands are IEEE fp16 instead of bf16 (set by launch_gemm from the precision)
  // 2-byte residual stream (round 5; half-precision engines only): `resid` and `out_f32` point to IEEE fp16 rows (ldr / ldc in
  // elements) instead of fp32 ones -- x <- fp16(x + A.W^T + b), the sum formed in fp32 and rounded once.  Served by the tiled
  // kernel, the ping-pong ring kernel and the weight-stationary kernel's residual form; the others refuse it.
  int x16 = 0;
  // x16 layers may also leave per-row LayerNorm partials of the rows they write (round 5: LayerNorm folded into the consumer
  // GEMM): row_part[b * part_ld + m] = float2(sum, sum of squares) of the STORED fp16 values of row m over the 32-column
  // block b (N / 32 blocks), every producer in the same association order (common.h ln_part4 / the epilogues' comments), so
  // that the statistics do not depend on which kernel served the layer.  Null: not written.
  float* row_part = nullptr;
  long part_ld = 0;
  // LayerNorm folded into the weight-stationary K = 512 GEMM (gemm_wreg.hip LNF): A = the raw fp16 residual rows, W = fp16
  // weights with the gain folded in and their rows centred (rowops.hip fold_ln_kernel), bias = b + W.beta, ln_stat = float2
  // (mean, rstd) per row of A
  const float* ln_stat = nullptr;
  // small launches: the statistics are formed inside the consumer from the producer's partials ([16][ln_part_ld] float2, what
  // ln_finalize_kernel would read; same arithmetic, bit-identical) -- only where gemm_wreg_stats_in_kernel(M, N) says so;
  // ln_stat must still be non-null (it selects the folded kernel) but is not read
  const float* ln_part = nullptr;
  long ln_part_ld = 0;
  // Full-row kernel (gemm_rowln, N = 512): out_f32 <- resid + A.W^T + bias and out_act <- LayerNorm(out_f32; ln_gamma,
  // ln_beta, ln_eps) from one launch.
  const float* ln_gamma = nullptr;
  const float* ln_beta = nullptr;
  float ln_eps = 0.f;
  // Deferred split-K reduce (round 6; BERT fc2 -> LayerNorm): when the launcher splits K, it leaves the slice sums in its slab
  // workspace and describes them here INSTEAD of launching splitk_reduce_kernel -- the caller's next kernel
  // (launch_layernorm_splitk) sums the slabs, adds bias and residual in the reduce kernel's order and normalises the row in one
  // pass.  pending->nslab == 0 after the call: the launch was not split, out_f32 holds the finished rows as usual.
  struct SplitkPending* splitk_pending = nullptr;
};
struct SplitkPending { const float* slabs = nullptr; int nslab = 0; long slab_stride = 0; int ld = 0; };
// Which kernel family served the calling thread's last launch_gemm / launch_gemm_rowln (g_gemm_family, common.h); GF_NONE: the
// launcher refused or M <= 0.  The values are part of include/conzic_hip_test.h (CZC_GEMM_FAMILY_*).
enum GemmFamily {
  GF_NONE = 0, GF_TILED_VEC = 1, GF_TILED_SCALAR = 2, GF_SPLITK = 3, GF_SKINNY = 4, GF_RING_LOADER = 5, GF_RING_PINGPONG = 6,
  GF_RING_SPLIT = 7, GF_WREG = 8, GF_WREG_LNF = 9, GF_WREG_RESID = 10, GF_ROWLN = 11
};
int launch_gemm(int prec, const GemmArgs& g, hipStream_t st);
bool gemm256_eligible(const GemmArgs& g);
int launch_gemm256(const GemmArgs& g, hipStream_t st);  // gemm256.hip: 256x256 LDS-DMA ring kernels (bf16 / fp16 operands)
extern int g_use_gemm256;  // 0 off, 1 default (ping-pong kernel for fp32 outputs, loader-wave kernel otherwise), 3 / 5 pin one of them
bool gemm256s_eligible(const GemmArgs& g);  // split-fp16 operands, same 256x256 persistent structure
int launch_gemm256s(const GemmArgs& g, hipStream_t st);
extern int g_use_gemm256s, g_gemm256s_min_m;
bool gemm_rowln_eligible(const GemmArgs& g);  // gemm256.hip: 128 x 512 full-row kernel, LayerNorm in the epilogue
int launch_gemm_rowln(const GemmArgs& g, hipStream_t st);
extern int g_rowln_min_m;
extern int g_use_skinny;
extern int g_use_splitk;
extern int g_gemm_deep;
extern int g_gemm_small_tiles;  // 128x128 kernel: two-deep operand prefetch 0 never / 1 for launches of <= one work-group per CU / 2 always
bool gemm_wreg_eligible(const GemmArgs& g);
int launch_gemm_wreg(const GemmArgs& g, hipStream_t st);  // gemm_wreg.hip: weights in registers, K = 512
// the same kernel with a residual epilogue on a 2-byte residual stream (K = 512, N % 256 == 0, x16): x <- fp16(x + A.W^T + b)
bool gemm_wreg_resid_eligible(const GemmArgs& g);
int launch_gemm_wreg_resid(const GemmArgs& g, hipStream_t st);
extern int g_use_wreg;
extern int g_wreg_resid_min_m;
extern int g_wreg_stats_in_kernel;  // 0: the folded consumer always takes its statistics from ln_finalize_kernel
bool gemm_wreg_stats_in_kernel(int M, int N);  // a folded launch of this shape can form its rows' statistics itself (GemmArgs::ln_part)
extern int g_wreg_min_m, g_gemm256_min_m;  // row-count thresholds of the two big-batch GEMM families

// ---- imageproc.hip ------------------------------------------------------------------------
// CLIP image geometry on the device, bit-identical to the PIL path of the reference's CLIPProcessor
size_t imageproc_scratch_bytes(int H, int W, int S);
int launch_clip_preprocess(const unsigned char* rgb_dev, int H, int W, int S, const float* mean, const float* stdv,
                           unsigned char* scratch, float* out, hipStream_t st);
// The same for N boxes of one resident image (a region = the contiguous copy of rgb[y0:y1, x0:x1] through the path above, bit
// for bit), one chunk per call: plan_clip_regions lays out the descriptors, the crop windows' coefficient tables (host
// arithmetic of the single-image path) and the intermediates; launch_clip_regions uploads plan.host in one copy and runs the
// two batched kernels, region r of the chunk into out + r * 3 * S * S.
struct RegionsPlan {
  std::vector<unsigned char> host;  // descriptors, then tables: the upload
  size_t tables_off = 0, tmp_off = 0, scratch_bytes = 0;
  int n = 0, max_rows = 0, any_h = 0;
};
int plan_clip_regions(int S, const int* boxes, int n, RegionsPlan& plan);
int launch_clip_regions(const unsigned char* rgb_dev, int W, int S, const RegionsPlan& plan, const float* mean, const float* stdv,
                        unsigned char* scratch, float* out, hipStream_t st);

// ---- rowops.hip -------------------------------------------------------------------------
// y = LN(x[row_idx ? row_idx[m] : m]) ; x fp32 [*,H]; outputs optional
// LayerNorm of rows that are still split-K slabs: v = slab_0 + slab_1 + ... (+ bias) (+ resid), in splitk_reduce_kernel's order, then
// launch_layernorm's arithmetic on v: bit-identical to the reduce kernel followed by the LayerNorm kernel (split-fp16 / f32 towers)
int launch_layernorm_splitk(int prec, const SplitkPending& sk, const float* bias, const float* resid, int ldr, const float* gamma,
                            const float* beta, float eps, int M, int H, void* y_act, float* y_f32, hipStream_t st);
int launch_layernorm(int prec, const float* x, const int* row_idx, const float* gamma, const float* beta, float eps,
                     int M, int H, void* y_act, float* y_f32, hipStream_t st);
// the same on a 2-byte residual stream: x16 = fp16 rows [*,512] (H must be 512, half-precision engines), y_act only
int launch_layernorm_x16(int prec, const void* x16, const int* row_idx, const float* gamma, const float* beta, float eps, int M,
                         int H, void* y_act, hipStream_t st);
// BERT embeddings: word + position + token_type(0) -> LN  (HF:bert/modeling_bert.py:98-106)
int launch_bert_embed(int prec, const int* ids, int B, int T, int H, const float* word, const float* pos,
                      const float* type0, const float* gamma, const float* beta, float eps, void* y_act, float* y_f32,
                      hipStream_t st);
// CLIP text embeddings on packed segments: x[own_off[s]+i] = tok[ids[src[s], pos0[s]+i]] + pos[pos0[s]+i]
// (HF:clip/modeling_clip.py:250-254)
int launch_clip_embed(const int* ids, int ids_stride, const int* seg_src, const int* seg_pos0, const int* own_off,
                      const int* own_len, int n_seg, int max_len, int H, const float* tok, const float* pos, float* x,
                      hipStream_t st, int x16 = 0, float* stat = nullptr, float eps = 0.f);  // x16: x is a 2-byte (fp16) residual stream; stat: float2 (mean, rstd) per row
// LayerNorm folded into the consumer GEMM: statistics from the producers' partials, one-time weight preparation
int launch_ln_finalize(const float* part, long part_ld, int nblk, int M, float eps, float* stat, hipStream_t st);
int launch_fold_ln(const float* W, const float* gamma, const float* beta, const float* b, int N, int K, void* Wf16, float* rowsum, float* bf,
                   hipStream_t st);
// vision: im2col of [B,3,S,S] into patches [B*P, 3*p*p] (act type), then assemble cls/pos
int launch_im2col(int prec, const float* pixels, int B, int S, int p, void* out, hipStream_t st);
int launch_vision_assemble(const float* patch_out, int B, int P, int H, const float* cls, const float* pos, float* x,
                           hipStream_t st);
int launch_convert(int prec, const float* src, void* dst, long n, hipStream_t st);  // fp32 -> act type
int launch_act_to_f32(int prec, const void* src, float* dst, long n, hipStream_t st);  // act type -> fp32
// gather rows: dst[m] = src[idx[m]]  (fp32 rows of width H)
int launch_gather_rows_f32(const float* src, const int* idx, int M, int H, float* dst, hipStream_t st);
int launch_gather_rows_bytes(const void* src, const int* idx, int M, int row_bytes, void* dst, hipStream_t st);
// rows b*T+gen_idx
int launch_make_row_index(int* idx, int B, int T, int gen_idx, hipStream_t st);
// rows b*T+gen[b] (gen: device, [B]; czc_generate_rows)
int launch_make_row_index_rows(int* idx, int B, int T, const int* gen, hipStream_t st);
// idx[s] = off[s] + len[s] - 1
int launch_eos_index(const int* off, const int* len, int n, int* idx, hipStream_t st);
int launch_l2_normalize(const float* x, int M, int D, float* y, hipStream_t st);
// inp[b, gen_idx .. gen_idx+n_mask) = mask_id
int launch_mask_positions(int* inp, int B, int T, int gen_idx, int n_mask, int mask_id, hipStream_t st);
// inp[b, gen[b] .. gen[b]+n_mask) = mask_id
int launch_mask_positions_rows(int* inp, int B, int T, const int* gen, int n_mask, int mask_id, hipStream_t st);
int launch_broadcast_rows_i32(const int* row, int T, int B, int* dst, hipStream_t st);
// dst[m] = src[idx[m]] for rows of W 4-byte words, any W
int launch_gather_rows_w32(const void* src, const int* idx, int M, int W, void* dst, hipStream_t st);
// czc_generate_rows_tied: for every row r with col[r] >= 0, inp[m][col[r]] = inp[r][col[r]] for the other members m of r's group
// (grp_of_row [R]; members of group g: grp_rows[grp_off[g] .. grp_off[g + 1]); all device)
int launch_tie_rows(int* inp, int R, int T, const int* col, const int* grp_of_row, const int* grp_off, const int* grp_rows, hipStream_t st);

// ---- ragged.hip (czc_generate_rows_len: BERT on packed ragged rows) -------------------------------------------------------
// Sequence b: row_len[b] tokens, packed rows row_off[b] .. (row_off [n + 1], the exclusive scan of row_len [n]; device).
// BERT embeddings + LN of the first row_len[b] ids of row run[b] (run null: row b) of ids [*, ids_stride] -> packed rows; token t
// of a sequence takes position embedding t.  max_T >= every row_len.  launch_bert_embed's arithmetic per row.
int launch_bert_embed_ragged(int prec, const int* ids, int ids_stride, const int* run, const int* row_off, const int* row_len, int n,
                             int max_T, int H, const float* word, const float* pos, const float* type0, const float* gamma,
                             const float* beta, float eps, void* y_act, float* y_f32, hipStream_t st);
// packed rows row_off[b] + gen[b] (gen: device, [n])
int launch_ragged_row_index(int* idx, int n, const int* row_off, const int* gen, hipStream_t st);

// ---- memo.hip (czc_generate option "memo") --------------------------------------------------------------------------
// check: hit[b] = (d_inp[b] with columns gen_idx .. gen_idx+n_mask-1 set to mask_id) == key[b]; list = the other images in
// ascending order; tot[0] = their count, tot[1 + j] = max over the hit images of img_max[j * B + b] (j < n_sub <= 2)
int launch_memo_check(const int* inp, int B, int T, int gen_idx, int n_mask, int mask_id, const int* key, const int* img_max,
                      int n_sub, int* hit, int* list, int* tot, hipStream_t st);
// for i < n, b = list ? list[i] : i: key[b] = masked row b; inp_c[i] = row b; img_c[i] = img_n[b] (each output may be null)
int launch_memo_gather(const int* inp, const int* list, int n, int T, int gen_idx, int n_mask, int mask_id, int* key, int* inp_c,
                       const float* img_n, int D, float* img_c, hipStream_t st);
// for i < n, b = list ? list[i] : i: (list) inp[b] = rows[i]; bcos_full[b] = bcos[i]; out_rows[b] = rows[i], out_cos[b] =
// bcos[i], out_max[b] = img_max[i] (each record may be null)
int launch_memo_scatter(const int* rows, const float* bcos, const int* img_max, const int* list, int n, int T, int* inp,
                        float* bcos_full, int* out_rows, float* out_cos, int* out_max, hipStream_t st);
// images with hit[b]: inp[b] = out_rows[b], bcos_full[b] = out_cos[b]
int launch_memo_fill(const int* hit, int B, int T, const int* out_rows, const float* out_cos, int* inp, float* bcos_full,
                     hipStream_t st);

// ---- memo_rows.hip (czc_generate_rows option "memo_rows") -----------------------------------------------------------
// The entries of one call: slot (p, r) = first position p of a step group (column - seed_len) x row r, L x R slots.
constexpr int MEMO_ROWS_SUB = 2;  // steps per group a slot has room for
struct MemoRowsTab {
  int* valid; int* sig;          // [L][R]: 1 once recorded in this call / the group shape it was recorded under
  int* key;                      // [L][R][T] masked row of the last visit
  int* rows; float* cos; int* imax;  // [L][MEMO_ROWS_SUB][R] x ([T] | 1 | 1): what each sub-step left
  int R, T, L, seed_len;
};
// col0 / col1 (device, [R]): every row's column at the group's first / second step (col1 null for a one-step group).
// A row that sits the group out (czc_generate_rows_from) has col0[r] = CZC_POS_IDLE.
// check: hit[r] = 1 where slot (col0[r] - seed_len, r) is valid, has this group's signature and its key row equals the masked
// row r, 2 where row r is idle, else 0; list = the rows with hit[r] == 0 in ascending order; tot[0] = their count, tot[1 + j] = max over the hit rows of the slot's imax at
// sub-step j (j < n_sub <= MEMO_ROWS_SUB); cnt: scratch, (R + 255) / 256 ints
// draw_rows (czc_generate_rows_draw; device, [R], may be null): a row with tau > 0 never hits -- its outcome is not a function
// of its masked row alone
struct RowDraw;
int launch_memo_rows_check(const int* inp, const MemoRowsTab& m, const int* col0, const int* col1, int n_mask0, int n_sub,
                           int mask_id, int* hit, int* cnt, int* list, int* tot, hipStream_t st, const RowDraw* draw_rows = nullptr);
// for i < n, r = list ? list[i] : i: (record) key of r's slot = masked row r, valid, signature; (inp_c) inp_c[i] = row r,
// img_c[i] = img_n[r], col_c[i] = col[r], dot_c[i] = dot[r] (col / dot: this step's schedule slice)
int launch_memo_rows_gather(const int* inp, const int* list, int n, const MemoRowsTab& m, const int* col0, const int* col1,
                            int n_mask0, int n_sub, int mask_id, int record, const int* col, const int* dot, int* inp_c,
                            const float* img_n, int D, float* img_c, int* col_c, int* dot_c, hipStream_t st);
// for i < n, r = list ? list[i] : i: (list) inp[r] = rows[i]; bcos_full[r] = bcos[i]; (record) sub-step j of r's slot =
// rows[i], bcos[i], img_max[i]
int launch_memo_rows_scatter(const int* rows, const float* bcos, const int* img_max, const int* list, int n, const MemoRowsTab& m,
                             const int* col0, int j, int record, int* inp, float* bcos_full, hipStream_t st);
// rows with hit[r] == 1: inp[r], bcos_full[r] = sub-step j of r's slot (idle rows are left alone)
int launch_memo_rows_fill(const int* hit, const MemoRowsTab& m, const int* col0, int j, int* inp, float* bcos_full, hipStream_t st);

// ---- attention.hip ------------------------------------------------------------------------
// Segment s = `own_len[s]` rows starting at own_off[s] (queries and keys/values) preceded by
// `pre_len[s]` key/value-only rows starting at pre_off[s] (the shared causal prefix of an image's
// candidates).  own_len == null: fixed-length segments s*fixed_T.. (BERT, vision).
struct SegTable {
  const int* pre_off; const int* pre_len; const int* own_off; const int* own_len;
  int n_seg; int fixed_T;
  // shared-prefix plans: longest branch (own rows of one candidate) of every image [B], or null.  The packed-branch
  // kernels take their packing factor from it PER IMAGE (32 / img_max[b] candidates per 32-query tile), so that an
  // image's attention arithmetic does not depend on which other images share its batch.
  const int* img_max = nullptr;
};
// softmax(q k^T * scale [+causal]) v; qkv [M, 3*heads*64] act type; out [M, heads*64] (own rows only)
int launch_attention(int prec, const void* qkv, const SegTable& tab, int max_keys, int heads, int causal, float scale,
                     void* out, hipStream_t st);
extern int g_use_mfma_attention;
extern int g_use_attention_image;
// bf16 engine, shared-prefix plan (B trunk segments then B*K branch segments): returns -1 when the
// shapes do not fit the packed-branch kernel (caller then uses launch_attention)
int launch_attention_shared(const void* qkv, const SegTable& tab, int B, int K, int max_own, int max_keys, int heads,
                            float scale, void* out, hipStream_t st, int f16 = 0);
// launch_attention_shared serves this plan with the per-image kernel (attention_image_kernel)
bool attention_image_serves(int B, int K, int max_own, int max_keys, int heads);
// such a plan in the tower's layer 0 on distinct rows: qkv [n_rows, 3*heads*64] holds packed branch row r at row rowmap[r] (trunk
// rows at their own indices); trunk and branch context rows are written at their packed indices
int launch_attention_shared_mapped(const void* qkv, int n_rows, const int* rowmap, const SegTable& tab, int B, int K, int max_own,
                                   int max_keys, int heads, float scale, void* out, hipStream_t st, int f16 = 0);
// such a plan in the tower's last layer: q from compact rows qc [B*K, heads*64] (one per candidate: q of its last own row), the
// context of those rows into compact rows ctx_c [B*K, heads*64]; k / v of all packed rows from qkv; no trunk rows are computed.
// rep [B*K] or null (launch_prefix_plan's table): a de-duplicated candidate gets the compact row of candidate rep[i] of its image.
int launch_attention_image_pooled(const void* qkv, const void* qc, const SegTable& tab, const int* rep, int B, int K, int max_own,
                                  int max_keys, int heads, float scale, void* ctx_c, hipStream_t st, int f16 = 0);

// the same for the split engine precision (qkv / out are split_t)
int launch_attention_shared_split(const void* qkv, const SegTable& tab, int B, int K, int max_own, int max_keys, int heads,
                                  float scale, void* out, hipStream_t st);

// ---- per-row hyper-parameters (czc_generate_rows_hp) ----------------------------------------------------------------------
// One record per row of a rows call, the layout of czc_hyper (engine.hip asserts it): uploaded once with the schedule and read
// by the four kernels that take hyper-parameters.  Those run one work-group per row (top-K, combine, refine_select) or one
// thread per candidate (bridge), so a row's record is uniform wherever a work-group reads it.
struct RowHyper { float alpha, beta, gamma, temperature; int control, negative; };

int launch_gather_row_hyper(const RowHyper* src, const int* idx, int n, RowHyper* dst, hipStream_t st);  // rowops.hip: dst[i] = src[idx[i]]

// ---- per-row seeded draw of the winner (czc_generate_rows_draw) -----------------------------------------------------------
// One record per row of a rows call, the layout of czc_draw on a little-endian host (engine.hip asserts it): the two halves of
// the row's 64-bit seed (the Philox key), its tau (0: the row keeps the first argmax) and the call's step offset.  Uploaded once
// with the schedule; read by the final combine (one work-group per row), the refine selection (a tau > 0 row is never
// margin-gated) and the rows memo's check (a tau > 0 row never hits).
struct RowDraw { unsigned seed_lo, seed_hi; float tau; unsigned step0; };

int launch_gather_row_draw(const RowDraw* src, const int* idx, int n, RowDraw* dst, hipStream_t st);  // rowops.hip: dst[i] = src[idx[i]]

// ---- topk.hip -----------------------------------------------------------------------------
int launch_softmax_mask_topk(const float* logits, int B, int V, int K, const float* mask, float temperature, int dot_id,
                             int dot_allowed, float* probs, int* idxs, int* cand, hipStream_t st);
// the same with the '.' rule per row: dot_rows[b] (device, [B]) in place of dot_allowed
int launch_softmax_mask_topk_rows(const float* logits, int B, int V, int K, const float* mask, float temperature, int dot_id,
                                  const int* dot_rows, float* probs, int* idxs, int* cand, hipStream_t st);
// the per-row form with the row's own temperature: hp_rows[b].temperature (device, [B]) in place of temperature
int launch_softmax_mask_topk_rows_hp(const float* logits, int B, int V, int K, const float* mask, const RowHyper* hp_rows, int dot_id,
                                     const int* dot_rows, float* probs, int* idxs, int* cand, hipStream_t st);
// the hyper-parameter form with a vocabulary set per row (czc_generate_rows_vocab): set_rows[b] (device, [B]) in [-1, n_sets) picks
// one of the bitsets bits [n_sets, W], W = ceil(V / 32); the mask factor of id i is mask[i] * bit(i), -1 = mask[i] alone
int launch_softmax_mask_topk_rows_vocab(const float* logits, int B, int V, int K, const float* mask, const RowHyper* hp_rows, int dot_id,
                                        const int* dot_rows, const int* set_rows, const unsigned* bits, int W, float* probs, int* idxs,
                                        int* cand, hipStream_t st);

// ---- bridge.hip ---------------------------------------------------------------------------
struct BridgeDev {
  int bert_vocab;
  const uint32_t* piece_off;
  const uint8_t* piece_bytes;
  const uint8_t* piece_class;
  const uint8_t* piece_flags;
  const int* byte_sym;
  const int* byte_sym_eow;
  const unsigned long long* hkeys;  // open addressing, ~0 = empty
  const unsigned long long* hvals;  // rank<<32 | out
  unsigned hmask;
  int bos_id, eos_id;
  // per BERT token: the CLIP ids of the token standing alone as a word (all-letter pieces whose byte-level BPE yields at
  // most BR_TOKMAX ids; tok_bpe_len 0 = not tabulated), filled once on the device by launch_bridge_precompute with the
  // same BPE code the per-row kernel runs.  May be null (every chunk then takes the merge loop).
  const int* tok_bpe = nullptr;
  const uint8_t* tok_bpe_len = nullptr;
};
constexpr int BR_TOKMAX = 8;
// fills tok_ids [bert_vocab * BR_TOKMAX] / tok_len [bert_vocab] (device buffers) from the uploaded tables of `bd`
int launch_bridge_precompute(const BridgeDev& bd, int* tok_ids, uint8_t* tok_len, hipStream_t st);
// rows: inp[b,:] with column gen_idx replaced by cand[b,k] (cand==null: rows are taken verbatim,
// n_rows = B, K = 1).  Writes clip_ids [B*K,77], clip_len, and optionally senti/repeats.
// Sentiment score of a row: sum of lexicon[id] over its non-special pieces, or -- when lex_pos [V][5] and
// lex_cls [V] are given -- sum of lex_pos[id][lex_cls[id]] over its word-start pieces.
// POS template for the control score (null tags = no POS score)
struct PosDev {
  const uint8_t* tag_of_token;  // [V]
  const uint16_t* masks;        // [n] accepted-tag bit masks, 0xFFFF = wildcard
  int n;
};
int launch_bridge(const BridgeDev& bd, const int* inp, int B, int T, int gen_idx, const int* cand, int K,
                  const float* lexicon, const float* lex_pos, const uint8_t* lex_cls, int negative, const PosDev& pos, int* clip_ids, int* clip_len, float* senti_raw,
                  float* repeats, int* overflow_flag, hipStream_t st);
// the same with the substituted column per row of inp: gen_rows[b] (device, [B]) in place of gen_idx (cand must not be null)
// row_len (device, [B]; czc_generate_rows_len) or null: row b holds row_len[b] tokens; the columns behind them are not read
// (neither decoded nor counted as repeats of a [PAD] candidate, nor scored)
int launch_bridge_rows(const BridgeDev& bd, const int* inp, int B, int T, const int* gen_rows, const int* cand, int K,
                       const float* lexicon, const float* lex_pos, const uint8_t* lex_cls, int negative, const PosDev& pos, int* clip_ids, int* clip_len,
                       float* senti_raw, float* repeats, int* overflow_flag, hipStream_t st, const int* row_len = nullptr);
// the per-row form with the control signal per row of inp: the launch is handed every table there is (each may be null) and the
// thread of a candidate of row b scores by hp_rows[b].control (1: lexicon / lex_pos with hp_rows[b].negative, 2: pos, 0: writes
// neither senti_raw nor repeats)
int launch_bridge_rows_hp(const BridgeDev& bd, const int* inp, int B, int T, const int* gen_rows, const int* cand, int K,
                          const float* lexicon, const float* lex_pos, const uint8_t* lex_cls, const RowHyper* hp_rows, const PosDev& pos,
                          int* clip_ids, int* clip_len, float* senti_raw, float* repeats, int* overflow_flag, hipStream_t st,
                          const int* row_len = nullptr);
// exclusive scan of len[n] -> off[n+1]; totals[0] = sum, totals[1] = max
int launch_scan(const int* len, int n, int* off, int* totals, hipStream_t st);
// Shared-prefix plan for B images x K candidates (segments: B trunks, then B*K branches):
//   p_b = share ? min(min_k LCP(ids[b,k], ids[b,0]), min_k len[b,k] - 1) : 0
//   trunk b: own_len p_b, src row b*K, pos0 0, pre_len 0;  branch (b,k): own_len len-p_b, src b*K+k, pos0 p_b, pre_len p_b
// max_len_out (two device ints, pre-zeroed) receive max len and max branch own_len via atomicMax.
int launch_prefix_plan(const int* clip_ids, const int* clip_len, int B, int K, int share, int* own_len, int* pre_len,
                       int* seg_src, int* seg_pos0, int* max_len_out, int* img_max, hipStream_t st,  // img_max [B]: longest branch per image
                       int* rep = nullptr, int* n_dup_out = nullptr);
// rep (optional, [B*K]): exact de-duplication -- rep[b*K+k] = lowest k' with an identical CLIP id row in image b (k itself for a
// first occurrence); the others get own_len 0 and pool their representative's EOS row; *n_dup_out += their number
// after the scan of own_len: pre_off[trunk] = 0, pre_off[branch (b,k)] = own_off[b];
// eos_idx[b*K+k] = own_off[B+b*K+k] + own_len[B+b*K+k] - 1
// Layer 0 on distinct rows (exact: the input of a packed row in layer 0 is token_embedding[id] + position_embedding[pos]): the
// representative of branch row (candidate k, offset i) of an image is the row at offset i of the lowest candidate of that image
// that has a row there holding the same CLIP id (all branches of an image start at the same position).  Trunk rows are their own.
// launch_layer0_count (plan phase, after launch_prefix_plan): distinct branch rows per image -> dcount [B], their sum added to
// *total.  launch_layer0_map (after launch_scan / launch_prefix_finish, sizes known): rowmap [M] = packed row -> index among the
// representative rows compacted in packed order (trunk rows first, indices kept), dist [n_trunk + sum] = the inverse list.
// Branches of more than 32 rows are outside the plans this serves (counted up to 32, never mapped).
int launch_layer0_count(const int* clip_ids, const int* own_len, const int* pre_len, int B, int K, int* dcount, int* total, hipStream_t st);
int launch_layer0_map(const int* clip_ids, const int* own_off, const int* own_len, const int* pre_len, const int* dcount, int B, int K,
                      int* rowmap, int* dist, hipStream_t st);
int launch_prefix_finish(const int* own_off, const int* own_len, int B, int K, int* pre_off, int* eos_idx,
                         int* n_trunk_rows, hipStream_t st, const int* rep = nullptr);

// ---- combine.hip --------------------------------------------------------------------------
struct CombineArgs {
  const float* text_feat;  // [B*K, D]
  const float* img_n;      // [B, D] L2-normalised
  float logit_scale_exp;
  const float* probs;      // [B,K]
  const int* cand;         // [B,K]
  const float* senti_raw;  // [B,K] or null
  const float* repeats;    // [B,K] or null
  float alpha, beta, gamma;
  int use_senti;           // 0 none, 1 sentiment (softmax(raw/1) + repeat penalty), 2 POS (softmax(raw/0.1))
  int B, K, D;
  float* clip_score; float* clip_ref; float* final_score;  // [B,K] (non-null, engine scratch)
  int* best; float* best_cos;                                // [B]
  int* inp; int T; int gen_idx;                              // write-back target (may be null)
  int* nonfinite = nullptr;                                  // set to 1 when a cosine is not finite (may be null)
  // screen-then-refine: candidates with refine_kind != 0 take their cosine from refine_cos (see combine.hip)
  const int* refine_kind = nullptr;                          // [B,K]
  const float* refine_cos = nullptr;                         // [B,K]
  // guard of the screen-then-refine scores: nonfinite[1] <- max over the re-encoded candidates of |screening error - its
  // estimated mean| (float bits), nonfinite[2] += images where that exceeds refine_guard (0 = no guard)
  float refine_guard = 0.f;
  // czc_generate_rows: the write-back column of row b is gen_rows[b] (device, [B]) instead of gen_idx; null = gen_idx
  const int* gen_rows = nullptr;
  // czc_generate_rows_hp: alpha, beta, gamma and use_senti (= control) of row b come from hp_rows[b] (device, [B]; needs
  // gen_rows); null = the scalars above
  const RowHyper* hp_rows = nullptr;
  // czc_generate_rows_draw: row b with draw_rows[b].tau > 0 draws its winner from softmax_K(final / tau) by the Gumbel-max rule
  // of combine.hip at step counter draw_rows[b].step0 + draw_step (device, [B]; needs gen_rows); null = first argmax
  const RowDraw* draw_rows = nullptr;
  unsigned draw_step = 0;
  // czc_generate_rows_vs: row b is also scored against the rival images rival_idx[b * M + j] (device, [B, M]; indices into
  // img_all, the whole normalised resident batch of n_img images [n_img, D]; -1 = empty slot, filled slots first).
  // disc [B*K] (device) receives P(own image | candidate) over {own} + rivals, and a row with rival_delta[b] != 0 and a filled
  // slot adds rival_delta[b] * disc to its fused score.  Needs gen_rows, hp_rows, draw_rows and text_feat; null = no rivals
  const int* rival_idx = nullptr;
  int M = 0;
  const float* rival_delta = nullptr;  // [B]
  const float* img_all = nullptr;
  int n_img = 0;
  float* disc = nullptr;
};
constexpr int CB_MAX_RIVALS = 16;       // CZC_MAX_RIVALS
constexpr int CB_RIVAL_FLOATS = 8192;   // the rival kernel's LDS array: D * CB_MAX_RIVALS floats at D = 512
// text_feat == null: clip_ref already holds the cosines
int launch_combine(const CombineArgs& a, hipStream_t st);
// the rival cosine kernel of launch_combine on its own (czc_score_rows_vs): cos_out as launch_cosine gives it, bit for bit, and
// disc [B*K] (1 for a row without a filled slot).  D * CB_MAX_RIVALS <= CB_RIVAL_FLOATS, M in [1, CB_MAX_RIVALS]
int launch_cosine_rival(const float* text_feat, const float* img_n, int B, int K, int D, const int* rival_idx, int M, const float* img_all,
                        int n_img, float logit_scale_exp, float* cos_out, float* disc, int* nonfinite, hipStream_t st);
// the cosine kernel of launch_combine on its own: cos_out[b * K + k] = normalised text_feat[b * K + k] . img_n[b]
int launch_cosine(const float* text_feat, const float* img_n, int B, int K, int D, float* cos_out, int* nonfinite, hipStream_t st);
// screen-then-refine engine (combine.hip): choose the candidates to re-encode / cosines of the re-encoded rows
// gate_h > 0: margin gate of czc_generate (combine.hip); gated[0] += images that passed it, gated[1] += images
int launch_refine_select(const float* clip_score, const float* final_score, int B, int K, float theta, int m_samples, float gate_h,
                         float beta, int need_cos, int* gated, int* kind, int* list, int* count, hipStream_t st);
// the same with beta and the mass threshold per row: beta = hp_rows[b].beta, theta = theta_base / max(beta * scale, 1e-6)
int launch_refine_select_rows(const float* clip_score, const float* final_score, int B, int K, float theta_base, float scale,
                              int m_samples, float gate_h, const RowHyper* hp_rows, int need_cos, int* gated, int* kind, int* list,
                              int* count, hipStream_t st);
// czc_generate_rows_draw: either form (hp_rows null: the scalar theta / beta) with the margin gate closed for the rows that
// draw (draw_rows[b].tau > 0): the gate proves an argmax, so such a row takes the full selection
int launch_refine_select_draw(const float* clip_score, const float* final_score, int B, int K, float theta, float theta_base, float scale,
                              int m_samples, float gate_h, float beta, const RowHyper* hp_rows, const RowDraw* draw_rows, int need_cos,
                              int* gated, int* kind, int* list, int* count, hipStream_t st);
int launch_refine_cosine(const float* text_feat, const float* img_n, const int* rlist, const int* n_rows_dev, int n_rows_max, int K, int D,
                         float* cos_out, int* nonfinite, hipStream_t st);
// segment plan of the refine pass (bridge.hip): B trunks (prefix lengths of the screening plan) + B x Kr branch slots
// (Kr = *kr_dev = the largest per-image count; an image's chosen candidates first, its other slots empty), i.e. the
// regular shape the packed-branch attention kernels take; rlist / eos_idx are compact (row r = count_off[b] + i)
int launch_refine_plan(const int* clip_len, const int* trunk_len, const int* list, const int* count, const int* count_off,
                       const int* kr_dev, int B, int K, int* own_len, int* pre_len, int* seg_src, int* seg_pos0, int* rlist,
                       int* max_len_out, int* img_max, hipStream_t st);
int launch_refine_finish(const int* own_off, const int* own_len, const int* count, const int* count_off, const int* kr_dev, int B, int K,
                         int* pre_off, int* eos_idx, hipStream_t st);

// ---- caption retrieval (retrieve.hip) ----------------------------------------------------------------------------------
// fp32 rows -> L2-normalised split_t rows, one pass; a row whose norm is 0 or not finite raises bad[row * bad_stride]
// (bad_stride = 0: one shared flag, only ever set) and is stored as zeros.  D % 32 == 0, D <= 1024.
int launch_normalize_split(const float* src, long n, int D, split_t* dst, int* bad, int bad_stride, hipStream_t st);
int index_scan_groups(int n, int D, int k, int groups);
// Q normalised split_t queries against n normalised split_t index rows: out_ids / out_cos [Q, k], ordered by (cosine descending,
// id ascending), tail (-1, -inf).  part: workspace of Q x G x k 8-byte keys, G = index_scan_groups(n, D, k, groups).
int launch_index_search(const split_t* index, int n, int D, const split_t* queries, int Q, int k, int G,
                        unsigned long long* part, int* out_ids, float* out_cos, hipStream_t st);

// ---- caption fluency (fluency.hip; czc_fluency_rows) -------------------------------------------------------------------------
// host: the expanded batch of R rows, one sequence per word -- sequence n masks column col_of_seq[n] = seed_len + j of row
// row_of_seq[n], rows in order and j ascending within a row (len_of_row null: every row has Lmax words).  Returns N = sum L_r;
// both arrays hold at least that many entries.
int fluency_expand_tables(int R, int seed_len, int Lmax, const int32_t* len_of_row, int32_t* row_of_seq, int32_t* col_of_seq);
// ids_out [N, T]: sequence n = row row_of_seq[n] of rows [*, T] with column col_of_seq[n] replaced by mask_id (every other
// column as it stands); target[n] = the id that stood there; gen_rows[n] = col_of_seq[n].  All device.
int launch_expand_mask_rows(const int* rows, int T, const int* row_of_seq, const int* col_of_seq, int N, int mask_id, int* ids_out,
                            int* target, int* gen_rows, hipStream_t st);
// logits [N, V] fp32, target [N] in [0, V), temperature > 0: logp[o] = log softmax(logits[n] / temperature)[target[n]] and
// rank[o] = #{i : x_i > x_t} + #{i < target : x_i == x_t} (raw logits; the order of topk.hip), o = out_idx ? out_idx[n] : n.
// One pass over the row.  A non-finite logp sets *nonfinite = 1.
int launch_logprob_target(const float* logits, int N, int V, const int* target, float temperature, const int* out_idx, float* logp,
                          int* rank, int* nonfinite, hipStream_t st);
// pll[r] = logp[r][0] + ... + logp[r][L_r - 1] in that order (logp [R, Lmax]; len_of_row device [R] or null: L_r = Lmax)
int launch_pll_sum(const float* logp, int R, int Lmax, const int* len_of_row, float* pll, hipStream_t st);

// ---- czc_internal_hooks (declared below, private to the build): what libconzic_hip_test.so may reach inside this library -----------
// The product library has hidden visibility; the hook library (api_test.hip) gets the launchers it wraps and the
// process-wide kernel-family switches it flips through this table instead of through exported C++ symbols.
constexpr int HOOKS_ABI = 0x060e;
struct Hooks {
  char* (*err_buf)();  // the calling host thread's g_err [512]
  decltype(&launch_gemm) gemm;
  decltype(&launch_gemm_rowln) gemm_rowln;
  decltype(&launch_layernorm) layernorm;
  decltype(&launch_convert) convert;
  decltype(&launch_act_to_f32) act_to_f32;
  decltype(&launch_attention) attention;
  decltype(&launch_attention_shared) attention_shared;
  decltype(&launch_attention_shared_split) attention_shared_split;
  decltype(&launch_softmax_mask_topk) softmax_mask_topk;
  decltype(&launch_bridge_precompute) bridge_precompute;
  decltype(&launch_bridge) bridge;
  decltype(&launch_l2_normalize) l2_normalize;
  decltype(&launch_combine) combine;
  decltype(&launch_layernorm_x16) layernorm_x16;
  decltype(&launch_ln_finalize) ln_finalize;
  decltype(&launch_fold_ln) fold_ln;
  decltype(&gemm_wreg_stats_in_kernel) wreg_stats_ok;
  int *use_gemm256, *use_skinny, *use_splitk, *gemm_deep, *gemm_small_tiles, *use_wreg, *use_gemm256s, *rowln_min_m,
      *wreg_min_m, *gemm256_min_m, *use_mfma_attention, *use_attention_image, *wreg_resid_min_m, *wreg_stats_in_kernel,
      *gemm256s_min_m;
  // the integer and selection side of the screen-then-refine engine (tests/test_refine_kernels_gpu.py)
  decltype(&launch_scan) scan;
  decltype(&launch_prefix_plan) prefix_plan;
  decltype(&launch_prefix_finish) prefix_finish;
  decltype(&launch_refine_select) refine_select;
  decltype(&launch_refine_select_rows) refine_select_rows;
  decltype(&launch_refine_select_draw) refine_select_draw;
  decltype(&launch_refine_plan) refine_plan;
  decltype(&launch_refine_finish) refine_finish;
  decltype(&launch_refine_cosine) refine_cosine;
  decltype(&launch_attention_image_pooled) attention_image_pooled;
  decltype(&launch_attention_shared_mapped) attention_shared_mapped;
  decltype(&launch_layer0_count) layer0_count;
  decltype(&launch_layer0_map) layer0_map;
  // the engine's text tower on host-given id rows (engine.hip test_text_tower; `engine` is a czc_engine*)
  int (*text_tower)(void* engine, const int32_t* clip_ids, const int32_t* clip_len, int B, int K, float* out, int32_t* n_dup);
  // the row, embedding, mover and memo kernels one by one (tests/test_row_kernels_gpu.py, tests/test_mover_memo_kernels_gpu.py)
  decltype(&launch_layernorm_splitk) layernorm_splitk;
  decltype(&launch_bert_embed) bert_embed;
  decltype(&launch_bert_embed_ragged) bert_embed_ragged;
  decltype(&launch_clip_embed) clip_embed;
  decltype(&launch_im2col) im2col;
  decltype(&launch_vision_assemble) vision_assemble;
  decltype(&launch_gather_rows_f32) gather_rows_f32;
  decltype(&launch_gather_rows_bytes) gather_rows_bytes;
  decltype(&launch_gather_rows_w32) gather_rows_w32;
  decltype(&launch_mask_positions) mask_positions;
  decltype(&launch_mask_positions_rows) mask_positions_rows;
  decltype(&launch_tie_rows) tie_rows;
  decltype(&launch_memo_check) memo_check;
  decltype(&launch_memo_gather) memo_gather;
  decltype(&launch_memo_scatter) memo_scatter;
  decltype(&launch_memo_fill) memo_fill;
  decltype(&launch_memo_rows_check) memo_rows_check;
  decltype(&launch_memo_rows_gather) memo_rows_gather;
  decltype(&launch_memo_rows_scatter) memo_rows_scatter;
  decltype(&launch_memo_rows_fill) memo_rows_fill;
  // caption fluency (tests/test_logprob_kernel_gpu.py, tests/test_expand_mask_gpu.py)
  decltype(&fluency_expand_tables) fluency_expand_tables;
  decltype(&launch_expand_mask_rows) expand_mask_rows;
  decltype(&launch_logprob_target) logprob_target;
  // the text bridge with candidates and the top-K selection in their per-row forms (tests/test_bridge_kernel_gpu.py against the
  // string reference tests/bridge_ref.py, pinned by tests/test_bridge_ref_cpu.py; tests/test_topk_rows_gpu.py)
  decltype(&launch_bridge_rows) bridge_rows;
  decltype(&launch_bridge_rows_hp) bridge_rows_hp;
  decltype(&launch_softmax_mask_topk_rows) softmax_mask_topk_rows;
  decltype(&launch_softmax_mask_topk_rows_hp) softmax_mask_topk_rows_hp;
  // the top-K selection with a vocabulary set per row (tests/test_topk_vocab_gpu.py)
  decltype(&launch_softmax_mask_topk_rows_vocab) softmax_mask_topk_rows_vocab;
  // the family the calling thread's last GEMM launch chose (GemmFamily; tests/test_gemm_layout_gpu.py)
  int (*gemm_family)();
  // the records a compact batch's combine reads (tests/test_combine_kernel_gpu.py)
  decltype(&launch_gather_row_hyper) gather_row_hyper;
  decltype(&launch_gather_row_draw) gather_row_draw;
};

}  // namespace czc

// The one door through which libconzic_hip_test.so (include/conzic_hip_test.h: kernel-level parity hooks for tests/ and the GEMM
// microbenchmark for tools/) reaches this library's kernel launchers and process-wide kernel-family switches.  NOT part of the
// drop-in boundary and not in include/conzic_hip.h: the symbol is exported (the hook library links against it), its table layout
// is private to the build.  Returns NULL when `abi` is not this build's tag.  Nothing on the product path calls it.
extern "C" __attribute__((visibility("default"))) const void* czc_internal_hooks(int abi);

