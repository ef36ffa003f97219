// Engine: frozen-weight residency, workspace, the three tower forwards and the polishing
// step/generate loops behind the C ABI of include/conzic_hip.h.
//
// One engine = one GPU = one HIP stream.  Weights are resident for the engine's lifetime
// (bf16 GEMM operands + fp32 LayerNorm/bias/embedding tables: ~0.75 GB of the 288 GB HBM);
// activations live in a grow-only workspace sized by the packed CLIP row count of the step.
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "../../include/conzic_hip.h"
#include "kernels.h"
#include "bridge_hash.h"

namespace czc {
thread_local char g_err[512] = {0};
thread_local int g_gemm_family = 0;
}
using namespace czc;

namespace {

struct Tensor {
  float* p = nullptr;
  std::vector<int64_t> shape;
  size_t numel = 0;
};

struct LayerW {
  void* qkv_w = nullptr; float* qkv_b = nullptr;
  void* o_w = nullptr; float* o_b = nullptr;
  float *ln1_g = nullptr, *ln1_b = nullptr;
  void* fc1_w = nullptr; float* fc1_b = nullptr;
  void* fc2_w = nullptr; float* fc2_b = nullptr;
  float *ln2_g = nullptr, *ln2_b = nullptr;
  // LayerNorm folded into the K = 512 GEMMs (bf16 engine's CLIP-text tower on the 2-byte residual stream): fp16 weights with
  // the gain folded in and their rows centred, bias + W.beta (rowops.hip fold_ln_kernel); null where the fold is not used
  void *qkv_wf = nullptr, *fc1_wf = nullptr;
  float *qkv_bf = nullptr, *fc1_bf = nullptr;
};

struct Buf {
  void* p = nullptr;
  size_t bytes = 0;
};

struct ProfKind {
  std::vector<hipEvent_t> ev;  // start/stop pairs
  size_t used = 0;
  double flops = 0;
  int64_t launches = 0;
};

// The per-row device records of a step (StepArgs::rec), one record per row of the batch the step runs on: the call's upload, or a
// compact batch's gather of it; all null outside a rows call.
// hp: czc_generate_rows_hp's hyper-parameters.  draw + step: czc_generate_rows_draw's records and the step's index in the call's
// schedule (the Philox counter is the record's step0 + step).  rival [rows, M] + delta [rows]: czc_generate_rows_vs' table and
// deltas; the indices point into img_all, the whole normalised resident batch of n_img images, which a compact batch leaves alone.
// vset [rows] + vbits [n_sets, vwords]: czc_generate_rows_vocab's set index of every row (-1: none) and the call's bitsets, which a
// compact batch leaves alone too; vhp [rows]: the records the top-K kernel reads the temperature from where the call's entries were
// all equal and hp is null (equal entries, so a compact batch takes its first rows as they are).
struct RowRecords {
  const RowHyper* hp = nullptr;
  const RowDraw* draw = nullptr; unsigned step = 0;
  const int* rival = nullptr; const float* delta = nullptr; int M = 0;
  const float* img_all = nullptr; int n_img = 0;
  const int* vset = nullptr; const unsigned* vbits = nullptr; int vwords = 0; const RowHyper* vhp = nullptr;
};

}  // namespace

struct czc_engine {
  czc_config cfg;
  int dev = 0;
  hipStream_t st = nullptr;
  bool shares_weights = false;  // czc_replicate: weights belong to the parent engine (which must outlive this one)
  hipEvent_t prof_ref = nullptr;  // recorded by czc_profile_reset: time zero of czc_profile_intervals
  char err[512] = {0};
  bool finalized = false;
  size_t esz = 2;  // bytes per CLIP activation element
  int pb = PREC_F32, pc = PREC_BF16;  // BERT / CLIP tower precisions
  int pv = PREC_BF16;                 // CLIP vision tower precision (= pc, except split-fp16 in the screen-then-refine engine)
  size_t eb = 4;   // bytes per BERT activation element
  // Screen-then-refine (CZC_PREC_REFINE): every candidate goes through the single-pass fp16 text tower; the candidates
  // that carry the softmax_K mass (+ a mass-stratified sample of the rest) are re-encoded by the split-fp16 tower
  // (ctext_x / tproj_wx) and the final scores are formed from the mixed cosines (combine.hip)
  bool refine = false;
  // mass threshold theta = refine_theta_x / (beta * exp(logit_scale)): 0.01 at beta 2, scale 100.  A candidate that keeps its
  // screening cosine moves its fused score by at most theta_x * |d_k - mean|: round 5 lowered theta_x from 4 to 2, so the
  // largest deviation measured (2.1e-4 over 256 k candidates) gives 4.2e-4 instead of 8.4e-4 of the 1e-3 bar
  float refine_theta_x = 2.0f;
  // czc_generate returns ids and winner cosines, not the K scores: its selection keeps round 3's threshold (4.0: fewer mass
  // carriers to re-encode; winners identical to the all-split engine on every validated image-step), the bound above is czc_step's
  float refine_theta_gen = 4.0f;
  int refine_samples = 12;      // strata of the sample among the candidates below the threshold, inside czc_generate
  // czc_step (all K fused scores are its output): twice the strata.  The sample's job is the mass-weighted MEAN screening error of
  // the candidates that keep their screening cosine; what is left of it after the correction scales the softmax denominator, and
  // through it the score of every re-encoded candidate by beta * p_k * exp(logit_scale) * (kept mass) * (error of the mean) -- the
  // largest term of czc_step's error on peaky images, and one the guard does not see.  Round 6, eleven weight draws x 2560
  // image-steps: worst fused-score difference 4.5e-4 .. 9.2e-4 with 12 strata, 2.8e-4 .. 5.4e-4 with 24 (profiles/r06_refine_samples_sweep.jsonl)
  int refine_samples_step = 24;
  // guard: the ~20 candidates an image re-encodes show their own |screening error - mean|; the candidates that keep their
  // screening cosine reach at most GUARD_RATIO = 2 times that sample maximum (fitted: 1.75 worst over 1280 image-steps), so
  // theta_x * 2 * sample_dev <= 1e-3 holds while sample_dev <= 2.5e-4 at theta_x = 2; trip point 0.8 of that
  float refine_guard_dev = 2.0e-4f;
  float guard_max_dev = 0.f; int64_t guard_trips = 0;   // since the last czc_refine_guard(reset = 1)
  // margin gate (czc_generate only; combine.hip refine_select_kernel): an image whose screening winner survives every
  // assignment of cosine errors |d_k - common| <= refine_gate_delta skips the second pass (its winner alone is re-encoded at
  // the snapshot steps, for the cosine the caller reads).  0 = off.  Default 4e-4 = 2x the largest |error - mean| measured
  // over 256 k candidates (2.1e-4), 2.7x the guard's sample maximum (1.5e-4)
  float refine_gate_delta = 4.0e-4f;
  // czc_generate's screening pass on the 2-byte residual stream with the LayerNorms folded into its GEMMs (the bf16 engine's
  // tower form, fp16 operands).  fp16 rows move its cosines: over the validation's candidates the guard's sample maximum
  // inside czc_generate grows from 1.3-1.6e-4 to 2.3-2.8e-4 (x1.72-1.76; the true maximum over all candidates of the
  // czc_step series from 2.1e-4 to 3.0e-4), so while it is on the three quantities that are bounds on that deviation move
  // together by refine_rows16_factor = 1.75: gate bound 7e-4, guard trip point 3.5e-4 (= bound / 2, as before) and the
  // selection's mass threshold theta_gen / 1.75 (theta * deviation, what a kept screening cosine can move a score by, stays).
  // czc_step keeps fp32 rows: all K fused scores are its output and fp16 rows would take its worst one from 6.3e-4 to 1.3e-3.
  int refine_rows16 = 1;
  float refine_rows16_factor = 1.75f;
  int64_t stat_gated = 0, stat_gate_images = 0;

  std::map<std::string, Tensor> w;
  std::vector<LayerW> bert, ctext, cvis, ctext_x;
  // extra processed weights
  void* mlm_dense_w = nullptr; void* decoder_w = nullptr; void* tproj_w = nullptr; void* vproj_w = nullptr;
  void* patch_w = nullptr; void* tproj_wx = nullptr;

  std::map<std::string, Buf> ws;
  float* d_mask = nullptr; int mask_vocab = 0;
  float* d_lex = nullptr;
  float* d_lex_pos = nullptr; uint8_t* d_lex_cls = nullptr;  // (word-start piece, coarse POS class) keyed table [V][5] + class per token
  uint8_t* d_pos_tags = nullptr; uint16_t* d_pos_masks = nullptr; int pos_n = 0;
  BridgeDev bd; bool has_bridge = false;
  std::vector<void*> bridge_allocs;
  float* d_img_n = nullptr; int img_B = 0;  // the resident image batch, L2-normalised [img_B, proj]: written only where it is set, encoded or freed
  float logit_scale_exp = 1.f;
  int* h_totals = nullptr;  // pinned, 64 ints: the blocks of the HT_* layout below
  int last_BT = 0, last_B = 0, last_T = 0;  // shape of the forward whose rows b_x / b_xg hold (n_mask = 0 re-use needs the same B AND T)
  int bert_prune = 1;       // last BERT layer behind the attention on the one row per sequence the MLM head reads (n_mask == 1 steps)
  int bert_pruned_idx = -1; // row the previous forward kept (-1: all rows of b_x are valid)
  // czc_generate_rows: the previous forward kept row bert_pruned_rows[b] of sequence b (bert_pruned_idx == PRUNED_ROWS); host
  // copy of that step's columns, valid inside the call only (null afterwards: nothing can re-use such a forward then)
  const int32_t* bert_pruned_rows = nullptr;
  int bert_fuse_splitk_ln = 1;  // BERT fc2: the LayerNorm kernel sums the split-K slabs itself (no reduce kernel); 0 = two kernels
  int share_prefix = 1;  // encode the candidates' common causal prefix once per image
  int dedup = 1;         // candidates of one image with identical CLIP id rows are encoded once (bridge.hip prefix_plan_kernel; exact)
  float* d_staged = nullptr; int staged_cap = 0, staged_n = 0;  // czc_preprocess_u8 output slots [cap][3][S][S]
  int pack_branches = 1; // pack several candidates' rows into one attention MFMA tile
  int pool_last_layer = 1; // last CLIP-text layer: out-proj + MLP on the EOS rows only
  int share_layer0 = 1;    // CLIP-text layer 0 on the folded path under the per-image attention kernel: q/k/v of every distinct (token, position) row once
  int pool_last_qkv = 1;   // ... and, on the folded path under the per-image attention kernel, q and the attention context too (k / v of all rows)
  int fuse_ln = 1;         // bf16 / fp16 CLIP-text tower: 1 = out-proj as a full-row kernel with LN2 in its epilogue
                           // (gemm_rowln_kernel; +1 % captions/s), 2 = fc2 -> next layer's LN1 as well (measured slower: the
                           // K = 2048 GEMM pays more for 128-row tiles than the LayerNorm pass costs), 0 = off
  // 2-byte residual stream of the CLIP-TEXT tower (round 5): x lives in HBM as IEEE fp16 rows (fp32 accumulate / bias /
  // residual add, one rounding per update), the out-projection runs on the weight-stationary kernel's residual form and the
  // LayerNorms read 1 KiB rows.  1 (default): the bf16 engine; 2: the single-pass fp16 tower too (CZC_PREC_FP16 and the
  // screening pass of CZC_PREC_REFINE: outside their validated error budget, experiments only); 0: fp32 residual everywhere.
  // The split-fp16 / f32 towers and the vision tower always keep the fp32 stream.
  int resid16 = 1;
  // with the 2-byte stream: LayerNorm folded into the q/k/v and fc1 GEMMs (they read x itself; statistics from the producer
  // GEMMs' partials; no LayerNorm kernel inside the stack).  0: LayerNorm kernels on the fp16 rows
  int fold_ln = 1;
  int prof = 0;  // 0 off, 1 every kernel class, 2 only the CLIP-text linear layers (the roofline kernel family)
  std::map<std::string, ProfKind> pk;
  int64_t stat_clip_rows = 0, stat_clip_seqs = 0, stat_bert_rows = 0, stat_steps = 0;
  int64_t stat_refine_rows = 0, stat_refine_seqs = 0;
  int64_t stat_dedup_seqs = 0;  // candidate sequences that rode on an identical one's rows (of stat_clip_seqs)
  // czc_set_control_callback: the host scores the K candidate sentences of every image itself (the reference's own
  // nltk scorer where it is installed) between the two halves of a step; replaces the table look-ups of the bridge kernel
  czc_control_fn ctl_fn = nullptr; void* ctl_user = nullptr;
  int32_t* h_ctl_ids = nullptr; float* h_ctl_scores = nullptr; size_t h_ctl_cap = 0;  // pinned: [B*T + B*K] ids, [B*K] scores
  // option "memo" (czc_generate only; memo.hip): a step runs only for the images whose masked row differs from the one they
  // had on their last visit of the same (position, n_mask) key in this call; the others take the entry's row and cosine back
  int memo = 0;
  int64_t stat_memo_hits = 0, stat_memo_images = 0;  // image-steps that took an entry / all image-steps of memo calls
  // option "memo_rows" (czc_generate_rows only; memo_rows.hip): the same rule keyed per row, with counters of its own
  int memo_rows = 0;
  int64_t stat_memo_row_hits = 0, stat_memo_row_steps = 0;  // row-steps that took an entry / all row-steps of memo_rows calls
  int32_t* h_memo_list = nullptr; size_t h_memo_list_cap = 0;  // pinned: the active rows of a checked step, read with their count
  // czc_index_set / czc_index_search (retrieve.hip): n L2-normalised text embeddings as split_t rows, this engine's own (a replica
  // has none); option "index_groups": work-groups of the scan, 0 = the launcher's choice
  split_t* d_index = nullptr; int64_t index_n = 0;
  int index_groups = 0;
  int fluency_chunk = 1024;  // czc_fluency_rows: expanded sequences per BERT forward (option "fluency_chunk", 1..16384)
  int regions_chunk = 64;    // czc_preprocess_regions_u8: regions per upload and launch pair (option "regions_chunk", 1..1024)
};

namespace {

constexpr int PRUNED_ROWS = 1 << 30;  // czc_engine::bert_pruned_idx: one row per sequence was kept, each sequence its own

#define E_CHECK(expr)                                                                         \
  do {                                                                                        \
    int _r = (expr);                                                                          \
    if (_r) {                                                                                 \
      if (!e->err[0]) snprintf(e->err, sizeof(e->err), "%s", czc::g_err);                     \
      return _r;                                                                              \
    }                                                                                         \
  } while (0)

#define E_HIP(expr)                                                                           \
  do {                                                                                        \
    hipError_t _h = (expr);                                                                   \
    if (_h != hipSuccess) {                                                                   \
      snprintf(e->err, sizeof(e->err), "%s:%d %s -> %s", __FILE__, __LINE__, #expr,           \
               hipGetErrorString(_h));                                                        \
      return CZC_ERR_HIP;                                                                     \
    }                                                                                         \
  } while (0)

int fail(czc_engine* e, int code, const char* fmt, const char* a = "") {
  snprintf(e->err, sizeof(e->err), fmt, a);
  return code;
}

int ensure(czc_engine* e, const char* name, size_t bytes, void** out) {
  Buf& b = e->ws[name];
  if (b.bytes < bytes) {
    if (b.p) {
      E_HIP(hipStreamSynchronize(e->st));
      E_HIP(hipFree(b.p));
    }
    size_t want = bytes + bytes / 4 + 256;
    E_HIP(hipMalloc(&b.p, want));
    b.bytes = want;
  }
  *out = b.p;
  return 0;
}

struct ProfScope {
  czc_engine* e;
  ProfKind* k = nullptr;
  ProfScope(czc_engine* e_, const char* kind, double flops) : e(e_) {
    if (!e->prof) return;
    // level 2: the CLIP-text tower only -- its linear layers (the roofline family) and its attention / row kernels
    if (e->prof == 2 && strncmp(kind, "gemm_clip_text", 14) != 0 && strcmp(kind, "gemm_clip_refine") != 0 &&
        !strstr(kind, "_clip_text")) return;
    k = &e->pk[kind];
    if (k->used + 2 > k->ev.size()) {
      for (int i = 0; i < 2; ++i) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) { k = nullptr; return; }
        k->ev.push_back(ev);
      }
    }
    k->flops += flops;
    k->launches += 1;
    (void)hipEventRecord(k->ev[k->used], e->st);
  }
  ~ProfScope() {
    if (!k) return;
    (void)hipEventRecord(k->ev[k->used + 1], e->st);
    k->used += 2;
  }
};

const Tensor* find(czc_engine* e, const std::string& n) {
  auto it = e->w.find(n);
  return it == e->w.end() ? nullptr : &it->second;
}

int need(czc_engine* e, const std::string& n, size_t numel, float** out) {
  const Tensor* t = find(e, n);
  if (!t) return fail(e, CZC_ERR_STATE, "missing tensor %s", n.c_str());
  if (t->numel != numel) return fail(e, CZC_ERR_STATE, "tensor %s has the wrong size", n.c_str());
  *out = t->p;
  return 0;
}

// GEMM operand in engine precision (new allocation); frees nothing
int to_act(czc_engine* e, int prec, const float* src, size_t numel, void** out) {
  void* p = nullptr;
  E_HIP(hipMalloc(&p, numel * prec_bytes(prec)));
  E_CHECK(launch_convert(prec, src, p, (long)numel, e->st));
  *out = p;
  return 0;
}

int build_layers(czc_engine* e, std::vector<LayerW>& L, int n_layers, int H, int I, bool bert_style,
                 const std::string& prefix, int prec) {
  const size_t es = prec_bytes(prec);
  L.resize(n_layers);
  for (int n = 0; n < n_layers; ++n) {
    LayerW& l = L[n];
    std::string p = prefix + std::to_string(n);
    std::string q, k, v, o, ln1, fc1, fc2, ln2;
    if (bert_style) {
      q = p + ".attention.self.query"; k = p + ".attention.self.key"; v = p + ".attention.self.value";
      o = p + ".attention.output.dense"; ln1 = p + ".attention.output.LayerNorm";
      fc1 = p + ".intermediate.dense"; fc2 = p + ".output.dense"; ln2 = p + ".output.LayerNorm";
    } else {
      q = p + ".self_attn.q_proj"; k = p + ".self_attn.k_proj"; v = p + ".self_attn.v_proj";
      o = p + ".self_attn.out_proj"; ln1 = p + ".layer_norm1";
      fc1 = p + ".mlp.fc1"; fc2 = p + ".mlp.fc2"; ln2 = p + ".layer_norm2";
    }
    float *qw, *kw, *vw, *qb, *kb, *vb, *t;
    E_CHECK(need(e, q + ".weight", (size_t)H * H, &qw));
    E_CHECK(need(e, k + ".weight", (size_t)H * H, &kw));
    E_CHECK(need(e, v + ".weight", (size_t)H * H, &vw));
    E_CHECK(need(e, q + ".bias", H, &qb));
    E_CHECK(need(e, k + ".bias", H, &kb));
    E_CHECK(need(e, v + ".bias", H, &vb));
    E_HIP(hipMalloc(&l.qkv_w, (size_t)3 * H * H * es));
    char* base = (char*)l.qkv_w;
    E_CHECK(launch_convert(prec, qw, base, (long)H * H, e->st));
    E_CHECK(launch_convert(prec, kw, base + (size_t)H * H * es, (long)H * H, e->st));
    E_CHECK(launch_convert(prec, vw, base + (size_t)2 * H * H * es, (long)H * H, e->st));
    E_HIP(hipMalloc((void**)&l.qkv_b, (size_t)3 * H * 4));
    E_HIP(hipMemcpyAsync(l.qkv_b, qb, (size_t)H * 4, hipMemcpyDeviceToDevice, e->st));
    E_HIP(hipMemcpyAsync(l.qkv_b + H, kb, (size_t)H * 4, hipMemcpyDeviceToDevice, e->st));
    E_HIP(hipMemcpyAsync(l.qkv_b + 2 * H, vb, (size_t)H * 4, hipMemcpyDeviceToDevice, e->st));
    E_CHECK(need(e, o + ".weight", (size_t)H * H, &t)); E_CHECK(to_act(e, prec, t, (size_t)H * H, &l.o_w));
    E_CHECK(need(e, o + ".bias", H, &l.o_b));
    E_CHECK(need(e, ln1 + ".weight", H, &l.ln1_g)); E_CHECK(need(e, ln1 + ".bias", H, &l.ln1_b));
    E_CHECK(need(e, fc1 + ".weight", (size_t)I * H, &t)); E_CHECK(to_act(e, prec, t, (size_t)I * H, &l.fc1_w));
    E_CHECK(need(e, fc1 + ".bias", I, &l.fc1_b));
    E_CHECK(need(e, fc2 + ".weight", (size_t)H * I, &t)); E_CHECK(to_act(e, prec, t, (size_t)H * I, &l.fc2_w));
    E_CHECK(need(e, fc2 + ".bias", H, &l.fc2_b));
    E_CHECK(need(e, ln2 + ".weight", H, &l.ln2_g)); E_CHECK(need(e, ln2 + ".bias", H, &l.ln2_b));
  }
  return 0;
}

int gemm_ex(czc_engine* e, int prec, const char* kind, const GemmArgs& g) {
  ProfScope ps(e, kind, 2.0 * g.M * (double)g.N * g.K);
  E_CHECK(launch_gemm(prec, g, e->st));
  return 0;
}

int gemm(czc_engine* e, int prec, const char* kind, const void* A, int lda, const void* W, int ldw, const float* bias,
         const float* resid, int ldr, void* out_act, float* out_f32, int ldc, int M, int N, int K, int act) {
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.resid = resid; g.ldr = ldr;
  g.out_act = out_act; g.out_f32 = out_f32; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.act = act;
  return gemm_ex(e, prec, kind, g);
}

// x <- fp16(x + A.W^T + b) on a 2-byte residual stream (GemmArgs::x16): x16 [M,N] fp16 rows, updated in place
// part (optional): LayerNorm partials of the rows written, [N / 32][part_ld] float2
int gemm_x16(czc_engine* e, int prec, const char* kind, const void* A, int lda, const void* W, const float* bias, void* x16, int M,
             int N, int K, float* part = nullptr, long part_ld = 0) {
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.bias = bias; g.resid = (const float*)x16; g.ldr = N;
  g.out_act = nullptr; g.out_f32 = (float*)x16; g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = ACT_NONE; g.x16 = 1;
  g.row_part = part; g.part_ld = part_ld;
  return gemm_ex(e, prec, kind, g);
}

// ---- layout of the pinned czc_engine::h_totals (64 ints) and of the device blocks that are copied into it ----
// HT_FLAG_PLAN: s_nonfinite[0] as read with a plan's totals (the previous steps' cosine check); HT_FLAGS: s_nonfinite as read at the end
// of a call (NF_*); HT_REFINE: the refine plan's totals (PT_*, RT_*); HT_MEMO: the step memo's check (MC_*); HT_PLAN: clip_plan's totals (PT_*)
enum : int { HT_FLAG_PLAN = 8, HT_FLAGS = 9, HT_REFINE = 16, HT_MEMO = 32, HT_PLAN = 48 };
// s_nonfinite: the cosine check, the refine guard's largest deviation (float bits) and trips, the margin gate's counts; NF_READ ints are read
enum : int { NF_NONFINITE = 0, NF_GUARD_DEV = 1, NF_GUARD_TRIPS = 2, NF_GATED = 4, NF_GATE_IMAGES = 5, NF_READ = 6 };
// a plan's device totals: rows, longest segment, text-bridge overflow, longest sequence, longest branch, de-duplicated candidates,
// trunk rows, causal (query, key) pairs, distinct branch rows of layer 0.  The refine plan has [0] [3] [4] [7] of them and RT_R =
// candidates to re-encode, RT_KR = the largest count of one image
enum : int { PT_ROWS = 0, PT_MAX_SEG = 1, PT_OVERFLOW = 2, PT_MAX_LEN = 3, PT_MAX_BRANCH = 4, PT_DUP = 5, PT_TRUNK = 6, PT_PAIRS = 7,
             PT_DIST = 8, RT_R = 8, RT_KR = 9 };
constexpr int PLAN_TOTALS = 48;  // bytes of a plan's device totals
enum : int { MC_ACTIVE = 0, MC_BRANCH0 = 1, MC_BRANCH1 = 2 };  // memo check: active images, longest branch of the HIT images at sub-step 0 / 1

// a plan's segment table and pooling indices on the device; rep: de-duplication table (null: none); dcount: layer 0's distinct rows per image (null: not counted)
struct PlanBufs { int *own_len, *pre_len, *src, *pos0, *own_off, *pre_off, *eidx, *img_max, *rep, *dcount; };

// Everything the text tower reads about a planned pass once its sizes have been read back: made by read_totals from clip_plan's
// totals and by the refine pass of step_phase_b from its own; the vision tower's stack runs on an empty one.
struct TowerPlan {
  PlanBufs buf{};
  int n_seg = 0, n_pool = 0, M = 0, max_len = 0, max_branch = 0;  // segments, sequences pooled at buf.eidx, packed rows, longest sequence / branch
  int B = 0, K = 0;          // regular B x K plan (B trunk segments, then B * K branches); 0: none
  int n_l0 = 0;              // layer 0 on distinct rows: trunk + distinct branch rows (0: not counted)
  int n_dup = 0;             // candidates that ride on an identical one's rows (the table: buf.rep)
  double pairs = 0;          // causal (query, key) pairs: attention FLOPs = 4 * H * pairs per layer
};

// a regular plan's branches go to the packed-branch attention kernels; a half-precision tower's to the per-image kernel where it
// serves the plan: the kernel whose mapped mode layer 0 and whose pooled mode the last layer may use
bool packed_branches(const czc_engine* e, const TowerPlan& tp) { return tp.B > 0 && g_use_mfma_attention && e->pack_branches; }
bool per_image_attention(const czc_engine* e, int P, const TowerPlan& tp) {
  return prec_is_half(P) && packed_branches(e, tp) && attention_image_serves(tp.B, tp.K, tp.max_branch, tp.max_len, e->cfg.clip_heads);
}

// ---- pre-LN transformer stack shared by the CLIP text and vision towers -----------------------
// layer 0 of the text tower on its distinct rows (kernels.h launch_layer0_map): n > 0 rows, dist [n] their packed rows, rowmap [M]
struct Layer0Rows { const int* rowmap = nullptr; const int* dist = nullptr; int n = 0; };
// P: precision of the layer weights L (an engine's CLIP precision, or PREC_F16X3 for the refine pass); gk: profile kind of the GEMMs.
// The residual stream x [M, H] is updated in place; tab describes its packed sequences (off / len, or fixed_T).
// Text tower only -- tp: its plan.  pool_idx: only these n_pool rows are needed after the stack (the EOS rows): the last layer runs
// its out-projection and MLP on them alone (K/V of every row are still produced) and returns the pooled residual rows in *pooled
// [n_pool, H].  r16: x (and *pooled) are fp16 rows of a 2-byte residual stream (czc_engine::resid16; H = 512, half-precision P).
// ln_stat0: (mean, rstd) of the incoming rows (embedding kernel): enables the LayerNorm fold.
struct StackDesc {
  int P; std::vector<LayerW>* L; const char* gk; int M, H, I, heads; float eps;
  SegTable tab; int max_keys, causal;
  TowerPlan tp; const int* pool_idx = nullptr; int n_pool = 0; bool r16 = false; const float* ln_stat0 = nullptr; Layer0Rows l0;
};

int clip_stack(czc_engine* e, const StackDesc& d, float* x, float** pooled = nullptr) {
  const int P = d.P, M = d.M, H = d.H, I = d.I, heads = d.heads, max_keys = d.max_keys, n_pool = d.n_pool;
  const float eps = d.eps; const bool r16 = d.r16; const char* gk = d.gk; const size_t esz = prec_bytes(P);
  const SegTable& tab = d.tab; const TowerPlan& tp = d.tp; const Layer0Rows& l0 = d.l0; std::vector<LayerW>& L = *d.L;
  void *y, *qkv, *ctx, *hbuf;
  E_CHECK(ensure(e, "cs_y", (size_t)M * H * esz, &y));
  E_CHECK(ensure(e, "cs_qkv", (size_t)M * 3 * H * esz, &qkv));
  E_CHECK(ensure(e, "cs_ctx", (size_t)M * H * esz, &ctx));
  E_CHECK(ensure(e, "cs_h", (size_t)M * I * esz, &hbuf));
  const float scale = 1.0f / sqrtf(64.0f);
  // the text tower's attention / row kernels are timed under their own classes (bench.py: MFMA utilisation of the whole
  // CLIP-text K-candidate batch, not only of its linear layers)
  const bool text = !strcmp(gk, "gemm_clip_text") || !strcmp(gk, "gemm_clip_refine");
  const char *ak = text ? "attention_clip_text" : "attention", *rk = text ? "rowops_clip_text" : "rowops";
  const double attn_flops = 4.0 * H * tp.pairs;  // (the vision tower has no plan: 0)
  // LayerNorm fused into the producer: out-proj (fuse_ln >= 1) and fc2 (fuse_ln >= 2) run on full 512-wide rows and
  // leave y = LN(x) beside the new fp32 x; the LayerNorm kernel then only runs where no such producer exists.
  const bool rowln = !r16 && prec_is_half(P) && e->fuse_ln && H == 512 && M >= g_rowln_min_m && I % 32 == 0;
  // LayerNorm folded into the q/k/v and fc1 GEMMs: they multiply x itself and correct with the row statistics `stat`, which
  // come from the producer's partials `part` (out-projection -> LN2, fc2 -> the next layer's LN1, the embedding kernel -> layer 0)
  const bool fold = r16 && e->fold_ln && !L.empty() && L[0].qkv_wf && d.ln_stat0;
  float *part = nullptr, *stat = nullptr;
  if (fold) E_CHECK(ensure(e, "cs_part", (size_t)(H / 32) * M * 8, (void**)&part));
  if (fold) E_CHECK(ensure(e, "cs_stat", (size_t)M * 8 + 256, (void**)&stat));
  // the statistics of `rows` rows for a folded consumer with N columns: stat <- (mean, rstd) from part -- unless the consumer is
  // small enough to form them itself (gemm_wreg_stats_in_kernel: one or two images), which saves this launch.  always: launch it
  // even then, for a reader of `stat` other than that consumer
  auto finalize = [&](int rows, int N, bool always = false) -> int {
    if (!always && gemm_wreg_stats_in_kernel(rows, N)) return 0;
    ProfScope ps(e, rk, 0);
    return launch_ln_finalize(part, M, H / 32, rows, eps, stat, e->st);
  };
  // st_: the rows' statistics; nullptr = what finalize(rows, N) left (in `stat`, or still in `part` for the consumer to sum)
  auto folded_gemm = [&](const void* Ax, const void* Wf, const float* bf, const float* st_, void* out, int rows, int N, int act, int ldc = 0) -> int {
    GemmArgs g;
    g.A = Ax; g.lda = H; g.W = Wf; g.ldw = H; g.bias = bf; g.resid = nullptr; g.ldr = 0; g.out_act = out; g.out_f32 = nullptr; g.ldc = ldc ? ldc : N;
    g.M = rows; g.N = N; g.K = H; g.act = act;
    g.ln_stat = st_ ? st_ : stat;
    if (!st_ && gemm_wreg_stats_in_kernel(rows, N)) { g.ln_part = part; g.ln_part_ld = M; g.ln_eps = eps; }
    return gemm_ex(e, P, gk, g);
  };
  auto ln = [&](const float* gm, const float* bt, int rows, const void* src, void* dst) -> int {  // dst <- LN(src rows)
    ProfScope ps(e, rk, 0);
    if (r16) return launch_layernorm_x16(P, src, nullptr, gm, bt, eps, rows, H, dst, e->st);
    return launch_layernorm(P, (const float*)src, nullptr, gm, bt, eps, rows, H, dst, nullptr, e->st);
  };
  auto resid_gemm = [&](const void* A, const void* W, const float* b, int K, float* xr, int rows) -> int {  // xr += A.W^T + b
    if (r16) return gemm_x16(e, P, gk, A, K, W, b, xr, rows, H, K);
    return gemm(e, P, gk, A, K, W, K, b, xr, H, nullptr, xr, H, rows, H, K, ACT_NONE);
  };
  auto resid_ln_gemm = [&](const void* A, const void* W, const float* b, int K, const float* gm, const float* bt) -> int {  // x += A.W^T + b; y = LN(x; gm, bt)
    GemmArgs g;
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.bias = b; g.resid = x; g.ldr = H; g.out_act = y; g.out_f32 = x;
    g.ldc = H; g.M = M; g.N = H; g.K = K; g.act = ACT_NONE; g.f16 = P == PREC_F16;
    g.ln_gamma = gm; g.ln_beta = bt; g.ln_eps = eps;
    ProfScope ps(e, gk, 2.0 * M * (double)H * K);
    return launch_gemm_rowln(g, e->st);
  };
  bool have_y = false;  // y already holds the next layer's LN1 output (left by this layer's fc2)
  // What follows a layer's attention, on `rows` rows (all M of x, or the pooled ones): xr += cx.Wo^T + b; xr += fc2(quick_gelu(fc1(LN2(xr))))
  // through yb / hb.  next: the layer that follows on these rows (null: none); it finds the partials of the new rows (folded path) or y (fuse_ln >= 2)
  // whole: the rows are the stream x itself (rows = M, yb = y), whose partials are M apart and which alone has the full-row kernels
  auto tail = [&](LayerW& l, bool whole, int rows, const void* cx, float* xr, void* yb, void* hb, const LayerW* next) -> int {
    if (fold) {
      E_CHECK(gemm_x16(e, P, gk, cx, H, l.o_w, l.o_b, xr, rows, H, H, part, M));
      E_CHECK(finalize(rows, I));
      E_CHECK(folded_gemm(xr, l.fc1_wf, l.fc1_bf, nullptr, hb, rows, I, ACT_QUICK_GELU));
      return gemm_x16(e, P, gk, hb, I, l.fc2_w, l.fc2_b, xr, rows, H, I, next ? part : nullptr, whole ? M : 0);
    }
    if (rowln && whole) E_CHECK(resid_ln_gemm(cx, l.o_w, l.o_b, H, l.ln2_g, l.ln2_b));  // (the full-row kernel is the whole stream's)
    else {
      E_CHECK(resid_gemm(cx, l.o_w, l.o_b, H, xr, rows));
      E_CHECK(ln(l.ln2_g, l.ln2_b, rows, xr, yb));
    }
    E_CHECK(gemm(e, P, gk, yb, H, l.fc1_w, H, l.fc1_b, nullptr, 0, hb, nullptr, I, rows, I, H, ACT_QUICK_GELU));
    have_y = rowln && whole && e->fuse_ln >= 2 && next;
    if (have_y) return resid_ln_gemm(hb, l.fc2_w, l.fc2_b, I, next->ln1_g, next->ln1_b);
    return resid_gemm(hb, l.fc2_w, l.fc2_b, I, xr, rows);
  };
  // Last layer, pooled rows only (pool_last_layer): out-projection and MLP on the n_pool gathered rows.  pool_qkv, on the folded path
  // under the per-image attention kernel: k / v of all rows, but q and the attention context too only of the pooled rows (every candidate's
  // last own row) -- the q/k/v GEMM as a k/v launch on M rows and a q launch on the gathered rows, the branch attention in its pooled mode,
  // no trunk attention.  Exact: a row of these GEMMs does not depend on the row count or the column split, a query column of the
  // attention tile only on its own q and the K/V tiles.
  const bool pool_last = d.pool_idx && e->pool_last_layer;
  const bool pool_qkv = pool_last && e->pool_last_qkv && fold && n_pool == tp.B * tp.K && per_image_attention(e, P, tp);
  for (size_t n = 0; n < L.size(); ++n) {
    LayerW& l = L[n];
    const bool last = n + 1 == L.size(), l0_rows = fold && n == 0 && l0.n > 0;
    const bool own_front = pool_qkv && last;  // q/k/v and the attention are the pooled layer's own (below)
    if (l0_rows) {
      // a packed row's input here is token_embedding[id] + position_embedding[pos]: q/k/v of every distinct row once, into the
      // first l0.n rows of qkv; the branch attention fetches row r at rowmap[r].  x stays packed (it is the residual).
      void* xg; float* sg;
      E_CHECK(ensure(e, "cs_xg", (size_t)l0.n * H * 2, &xg));
      E_CHECK(ensure(e, "cs_sg", (size_t)l0.n * 8 + 256, (void**)&sg));
      { ProfScope ps(e, rk, 0);
        E_CHECK(launch_gather_rows_bytes(x, l0.dist, l0.n, H * 2, xg, e->st));
        E_CHECK(launch_gather_rows_w32(d.ln_stat0, l0.dist, l0.n, 2, sg, e->st)); }
      E_CHECK(folded_gemm(xg, l.qkv_wf, l.qkv_bf, sg, qkv, l0.n, 3 * H, ACT_NONE));
    } else if (fold && !own_front) {
      E_CHECK(folded_gemm(x, l.qkv_wf, l.qkv_bf, n == 0 ? d.ln_stat0 : nullptr, qkv, M, 3 * H, ACT_NONE));
    } else if (!fold) {
      if (!have_y) E_CHECK(ln(l.ln1_g, l.ln1_b, M, x, y));
      E_CHECK(gemm(e, P, gk, y, H, l.qkv_w, H, l.qkv_b, nullptr, 0, qkv, nullptr, 3 * H, M, 3 * H, H, ACT_NONE));
    }
    if (!own_front) {
      ProfScope ps(e, ak, attn_flops);
      int rc = -1;
      if (l0_rows)
        rc = launch_attention_shared_mapped(qkv, l0.n, l0.rowmap, tab, tp.B, tp.K, tp.max_branch, max_keys, heads, scale, ctx, e->st, P == PREC_F16);
      else if (prec_is_half(P) && packed_branches(e, tp))
        rc = launch_attention_shared(qkv, tab, tp.B, tp.K, tp.max_branch, max_keys, heads, scale, ctx, e->st, P == PREC_F16);
      else if (P == PREC_F16X3 && packed_branches(e, tp))
        rc = launch_attention_shared_split(qkv, tab, tp.B, tp.K, tp.max_branch, max_keys, heads, scale, ctx, e->st);
      if (rc > 0) E_CHECK(rc);
      if (rc < 0) E_CHECK(launch_attention(P, qkv, tab, max_keys, heads, d.causal, scale, ctx, e->st));
    }
    if (pool_last && last) {
      // the pooled rows' context, q (pool_qkv) or LN2 output, hidden and residual rows, and their gathered statistics (pool_qkv)
      void *ctx_e, *qy_e, *h_e; float *x_e, *stat_e = nullptr;
      E_CHECK(ensure(e, "cs_ctx_e", (size_t)n_pool * H * esz, &ctx_e));
      E_CHECK(ensure(e, pool_qkv ? "cs_q_e" : "cs_y_e", (size_t)n_pool * H * esz, &qy_e));
      E_CHECK(ensure(e, "cs_h_e", (size_t)n_pool * I * esz, &h_e));
      E_CHECK(ensure(e, "cs_x_e", (size_t)n_pool * H * 4, (void**)&x_e));
      if (pool_qkv) {
        E_CHECK(ensure(e, "cs_stat_e", (size_t)n_pool * 8 + 256, (void**)&stat_e));
        const float* st_all = n == 0 ? d.ln_stat0 : stat;  // layer n - 1 left them finalized (below)
        { ProfScope ps(e, rk, 0);
          E_CHECK(launch_gather_rows_bytes(x, d.pool_idx, n_pool, H * 2, x_e, e->st));
          E_CHECK(launch_gather_rows_w32(st_all, d.pool_idx, n_pool, 2, stat_e, e->st)); }
        E_CHECK(folded_gemm(x, (const char*)l.qkv_wf + (size_t)H * H * 2, l.qkv_bf + H, st_all, (char*)qkv + (size_t)H * esz, M, 2 * H,
                            ACT_NONE, 3 * H));
        E_CHECK(folded_gemm(x_e, l.qkv_wf, l.qkv_bf, stat_e, qy_e, n_pool, H, ACT_NONE));
        ProfScope ps(e, ak, attn_flops);
        E_CHECK(launch_attention_image_pooled(qkv, qy_e, tab, tp.buf.rep, tp.B, tp.K, tp.max_branch, max_keys, heads, scale, ctx_e, e->st,
                                              P == PREC_F16));
      } else {
        ProfScope ps(e, rk, 0);
        E_CHECK(launch_gather_rows_bytes(ctx, d.pool_idx, n_pool, H * (int)esz, ctx_e, e->st));
        if (r16) E_CHECK(launch_gather_rows_bytes(x, d.pool_idx, n_pool, H * 2, x_e, e->st));
        else E_CHECK(launch_gather_rows_f32(x, d.pool_idx, n_pool, H, x_e, e->st));
      }
      E_CHECK(tail(l, false, n_pool, ctx_e, x_e, qy_e, h_e, nullptr));
      *pooled = x_e;
      return 0;
    }
    E_CHECK(tail(l, true, M, ctx, x, y, hbuf, last ? nullptr : &L[n + 1]));  // (the last layer's rows only feed the final LayerNorm)
    // a pooled last layer (pool_qkv) gathers the statistics of its rows: always in `stat`, not left in `part` for a consumer to sum
    if (fold && !last) E_CHECK(finalize(M, 3 * H, pool_qkv && n + 2 == L.size()));
  }
  return 0;
}

// czc_generate_rows_len: the B sequences of a step have their own lengths.  off [B + 1] / len [B] (device): sequence b has len[b]
// tokens -- the first len[b] columns of row b of the [B, T] strided ids -- and packed rows off[b] ..; M = off[B], max_T = the
// longest.  Null wherever a Ragged* is taken: B x T rows, the uniform path.
struct Ragged { const int* off; const int* len; int M; int max_T; };

// ---- BERT encoder (post-LN) on [B*T] rows: leaves the final hidden state in ws "b_x" ----------
// keep_idx >= 0: only row keep_idx of every sequence is read afterwards (the masked slot, gen_utils.py:69): the last layer
// still forms q/k/v and the attention for all rows, then gathers that row and runs out-proj / LN / MLP / LN on B rows
// instead of B*T; the result goes to ws "b_xg" [B,H].  Same kernels per row, so the row's values do not change.
// keep_rows (device, [B]; with keep_rows_host its host copy): the kept row is keep_rows[b] of sequence b (czc_generate_rows).
// rag: the stack runs on the rag->M packed rows of ragged sequences (ragged.hip embedding, attention over each sequence's own
// keys, kept row rag->off[b] + keep_rows[b]); the GEMMs and LayerNorms are the same launches on M rows.
int bert_forward(czc_engine* e, const int* d_inp, int B, int T, int keep_idx = -1, const int* keep_rows = nullptr,
                 const int32_t* keep_rows_host = nullptr, const Ragged* rag = nullptr) {
  const czc_config& c = e->cfg;
  const int P = e->pb, M = rag ? rag->M : B * T, H = c.bert_hidden, I = c.bert_inter;
  if (rag && keep_idx >= 0 && !keep_rows) return fail(e, CZC_ERR_STATE, "ragged BERT rows keep a row per sequence (keep_rows)%s");
  void *xa, *qkv, *ctx, *hbuf; float *x, *tmp;
  E_CHECK(ensure(e, "b_x", (size_t)M * H * 4, (void**)&x));
  E_CHECK(ensure(e, "b_tmp", (size_t)M * H * 4, (void**)&tmp));
  E_CHECK(ensure(e, "b_xa", (size_t)M * H * e->eb, &xa));
  E_CHECK(ensure(e, "b_qkv", (size_t)M * 3 * H * e->eb, &qkv));
  E_CHECK(ensure(e, "b_ctx", (size_t)M * H * e->eb, &ctx));
  E_CHECK(ensure(e, "b_h", (size_t)M * I * e->eb, &hbuf));
  float *word, *pos, *typ, *g, *b;
  E_CHECK(need(e, "bert.embeddings.word_embeddings.weight", (size_t)c.bert_vocab * H, &word));
  E_CHECK(need(e, "bert.embeddings.position_embeddings.weight", (size_t)c.bert_max_pos * H, &pos));
  E_CHECK(need(e, "bert.embeddings.token_type_embeddings.weight", (size_t)2 * H, &typ));
  E_CHECK(need(e, "bert.embeddings.LayerNorm.weight", H, &g));
  E_CHECK(need(e, "bert.embeddings.LayerNorm.bias", H, &b));
  { ProfScope ps(e, "rowops", 0);
    if (rag) E_CHECK(launch_bert_embed_ragged(P, d_inp, T, nullptr, rag->off, rag->len, B, rag->max_T, H, word, pos, typ, g, b, c.bert_eps, xa, x, e->st));
    else E_CHECK(launch_bert_embed(P, d_inp, B, T, H, word, pos, typ, g, b, c.bert_eps, xa, x, e->st)); }
  const float scale = 1.0f / sqrtf(64.0f);
  e->bert_pruned_idx = -1;
  e->bert_pruned_rows = nullptr;
  // fc2 + residual + LayerNorm (HF:bert/modeling_bert.py:488-496): xr <- LN(xr + h.W2^T + b), xa <- the same in the operand type.
  // Where the launcher splits K (fc2's K = 3072 at every row count above the skinny kernel's 32) the slice sums stay in its slab
  // workspace and the LayerNorm kernel sums them itself (GemmArgs::splitk_pending): one launch less per layer, no fp32 round trip
  auto fc2_ln = [&](const void* h, LayerW& l, float* xr, int rows) -> int {
    SplitkPending pend;
    GemmArgs g;
    g.A = h; g.lda = I; g.W = l.fc2_w; g.ldw = I; g.bias = l.fc2_b; g.resid = xr; g.ldr = H; g.out_act = nullptr; g.out_f32 = tmp; g.ldc = H;
    g.M = rows; g.N = H; g.K = I; g.act = ACT_NONE;
    g.splitk_pending = e->bert_fuse_splitk_ln ? &pend : nullptr;
    E_CHECK(gemm_ex(e, P, "gemm_bert", g));
    ProfScope ps(e, "rowops", 0);
    if (pend.nslab > 0) E_CHECK(launch_layernorm_splitk(P, pend, l.fc2_b, xr, H, l.ln2_g, l.ln2_b, c.bert_eps, rows, H, xa, xr, e->st));
    else E_CHECK(launch_layernorm(P, tmp, nullptr, l.ln2_g, l.ln2_b, c.bert_eps, rows, H, xa, xr, e->st));
    return 0;
  };
  for (int n = 0; n < c.bert_layers; ++n) {
    LayerW& l = e->bert[n];
    E_CHECK(gemm(e, P, "gemm_bert", xa, H, l.qkv_w, H, l.qkv_b, nullptr, 0, qkv, nullptr, 3 * H, M, 3 * H, H, ACT_NONE));
    { ProfScope ps(e, "attention", 0);
      SegTable tab{nullptr, nullptr, rag ? rag->off : nullptr, rag ? rag->len : nullptr, B, rag ? 0 : T};
      E_CHECK(launch_attention(P, qkv, tab, rag ? rag->max_T : T, c.bert_heads, 0, scale, ctx, e->st)); }
    if (keep_idx >= 0 && n + 1 == c.bert_layers) {
      int* idx; void* ctx_g; float* x_g;
      E_CHECK(ensure(e, "b_pidx", (size_t)B * 4, (void**)&idx));
      E_CHECK(ensure(e, "b_cg", (size_t)B * H * e->eb, &ctx_g));
      E_CHECK(ensure(e, "b_xg", (size_t)B * H * 4, (void**)&x_g));
      { ProfScope ps(e, "rowops", 0);
        if (rag) E_CHECK(launch_ragged_row_index(idx, B, rag->off, keep_rows, e->st));
        else if (keep_rows) E_CHECK(launch_make_row_index_rows(idx, B, T, keep_rows, e->st));
        else E_CHECK(launch_make_row_index(idx, B, T, keep_idx, e->st));
        E_CHECK(launch_gather_rows_bytes(ctx, idx, B, H * (int)e->eb, ctx_g, e->st));
        E_CHECK(launch_gather_rows_f32(x, idx, B, H, x_g, e->st)); }
      // tmp / xa / hbuf: their first B rows are free here (xa fed this layer's q/k/v, hbuf the previous layer's fc2)
      E_CHECK(gemm(e, P, "gemm_bert", ctx_g, H, l.o_w, H, l.o_b, x_g, H, nullptr, tmp, H, B, H, H, ACT_NONE));
      { ProfScope ps(e, "rowops", 0); E_CHECK(launch_layernorm(P, tmp, nullptr, l.ln1_g, l.ln1_b, c.bert_eps, B, H, xa, x_g, e->st)); }
      E_CHECK(gemm(e, P, "gemm_bert", xa, H, l.fc1_w, H, l.fc1_b, nullptr, 0, hbuf, nullptr, I, B, I, H, ACT_GELU_ERF));
      E_CHECK(fc2_ln(hbuf, l, x_g, B));
      e->bert_pruned_idx = keep_rows ? PRUNED_ROWS : keep_idx;
      e->bert_pruned_rows = keep_rows ? keep_rows_host : nullptr;
      break;
    }
    E_CHECK(gemm(e, P, "gemm_bert", ctx, H, l.o_w, H, l.o_b, x, H, nullptr, tmp, H, M, H, H, ACT_NONE));
    { ProfScope ps(e, "rowops", 0); E_CHECK(launch_layernorm(P, tmp, nullptr, l.ln1_g, l.ln1_b, c.bert_eps, M, H, xa, x, e->st)); }
    E_CHECK(gemm(e, P, "gemm_bert", xa, H, l.fc1_w, H, l.fc1_b, nullptr, 0, hbuf, nullptr, I, M, I, H, ACT_GELU_ERF));
    E_CHECK(fc2_ln(hbuf, l, x, M));
  }
  return 0;
}

// MLM head on row gen_idx of every sequence -> logits fp32 [B,V] in ws "b_logits"
// gen_rows (device, [B]) / gen_rows_host: row gen_rows[b] of sequence b instead (czc_generate_rows)
int mlm_head(czc_engine* e, int B, int T, int gen_idx, float** logits_out, const int* gen_rows = nullptr,
             const int32_t* gen_rows_host = nullptr, const Ragged* rag = nullptr) {
  const czc_config& c = e->cfg;
  const int P = e->pb, H = c.bert_hidden, V = c.bert_vocab;
  float* x = (float*)e->ws["b_x"].p;
  int* idx; float *gx, *t32, *logits; void *ga, *ta;
  E_CHECK(ensure(e, "h_idx", (size_t)B * 4, (void**)&idx));
  E_CHECK(ensure(e, "h_gx", (size_t)B * H * 4, (void**)&gx));
  E_CHECK(ensure(e, "h_ga", (size_t)B * H * e->eb, &ga));
  E_CHECK(ensure(e, "h_t32", (size_t)B * H * 4, (void**)&t32));
  E_CHECK(ensure(e, "h_ta", (size_t)B * H * e->eb, &ta));
  E_CHECK(ensure(e, "b_logits", (size_t)B * V * 4, (void**)&logits));
  float *db, *g, *b, *bias;
  E_CHECK(need(e, "cls.predictions.transform.dense.bias", H, &db));
  E_CHECK(need(e, "cls.predictions.transform.LayerNorm.weight", H, &g));
  E_CHECK(need(e, "cls.predictions.transform.LayerNorm.bias", H, &b));
  E_CHECK(need(e, "cls.predictions.bias", V, &bias));
  // the rule holds per row: every sequence must read the one row its forward kept
  const bool kept_same = gen_rows ? (e->bert_pruned_idx == PRUNED_ROWS && e->bert_pruned_rows && gen_rows_host &&
                                     !memcmp(e->bert_pruned_rows, gen_rows_host, (size_t)B * 4))
                                  : e->bert_pruned_idx == gen_idx;
  if (e->bert_pruned_idx >= 0 && !kept_same)
    return fail(e, CZC_ERR_STATE, "n_mask=0 re-use of a forward that kept one row only (it follows an n_mask >= 2 step, gen_utils.py:164-166)%s");
  { ProfScope ps(e, "rowops", 0);
    if (e->bert_pruned_idx >= 0) {
      gx = (float*)e->ws["b_xg"].p;  // the forward left exactly these rows
    } else {
      if (rag && !gen_rows) return fail(e, CZC_ERR_STATE, "ragged BERT rows are read by a row per sequence (gen_rows)%s");
      if (rag) E_CHECK(launch_ragged_row_index(idx, B, rag->off, gen_rows, e->st));
      else if (gen_rows) E_CHECK(launch_make_row_index_rows(idx, B, T, gen_rows, e->st));
      else E_CHECK(launch_make_row_index(idx, B, T, gen_idx, e->st));
      E_CHECK(launch_gather_rows_f32(x, idx, B, H, gx, e->st));
    }
    E_CHECK(launch_convert(P, gx, ga, (long)B * H, e->st)); }
  E_CHECK(gemm(e, P, "gemm_bert", ga, H, e->mlm_dense_w, H, db, nullptr, 0, nullptr, t32, H, B, H, H, ACT_GELU_ERF));
  { ProfScope ps(e, "rowops", 0); E_CHECK(launch_layernorm(P, t32, nullptr, g, b, c.bert_eps, B, H, ta, nullptr, e->st)); }
  E_CHECK(gemm(e, P, "gemm_bert", ta, H, e->decoder_w, H, bias, nullptr, 0, nullptr, logits, V, B, V, H, ACT_NONE));
  *logits_out = logits;
  return 0;
}

// CLIP text tower (clip/clip.py:78-83) on B x K candidate sequences: ids [B*K,77] + len -> feat fp32
// [B*K, proj].  With `share` the causal prefix common to an image's K candidates is encoded once
// (trunk segment) and every candidate only carries the rows from its first differing token on.
// Two halves around the step's single host round trip (32 bytes of totals: rows, longest sequence, overflow):
// clip_plan builds the segment table on the device and starts the read, clip_tower runs on the sizes it returned.
// the refine engine inside czc_generate (in_generate: StepMode): screening pass on fp16 rows (czc_engine::refine_rows16)
static inline bool refine_rows16_now(const czc_engine* e, bool in_generate) {
  return e->refine && in_generate && e->refine_rows16 && e->cfg.clip_hidden == 512;
}

// pfx "p": the plan of the screening / only pass; "r": the plan of the refine pass
int plan_bufs(czc_engine* e, int B, int K, PlanBufs* p, const char* pfx = "p") {
  const int n_seq = B * K, S = B + n_seq;
  const std::string q(pfx);
  E_CHECK(ensure(e, (q + "_own_len").c_str(), (size_t)S * 4, (void**)&p->own_len));
  E_CHECK(ensure(e, (q + "_pre_len").c_str(), (size_t)S * 4, (void**)&p->pre_len));
  E_CHECK(ensure(e, (q + "_src").c_str(), (size_t)S * 4, (void**)&p->src));
  E_CHECK(ensure(e, (q + "_pos0").c_str(), (size_t)S * 4, (void**)&p->pos0));
  E_CHECK(ensure(e, (q + "_own_off").c_str(), (size_t)(S + 1) * 4, (void**)&p->own_off));
  E_CHECK(ensure(e, (q + "_pre_off").c_str(), (size_t)S * 4, (void**)&p->pre_off));
  E_CHECK(ensure(e, (q + "_eidx").c_str(), (size_t)n_seq * 4, (void**)&p->eidx));
  E_CHECK(ensure(e, (q + "_img_max").c_str(), (size_t)B * 4, (void**)&p->img_max));
  E_CHECK(ensure(e, (q + "_rep").c_str(), (size_t)n_seq * 4, (void**)&p->rep));
  p->dcount = nullptr;
  return 0;
}

// *bufs: what the plan filled (rep / dcount: null without de-duplication / where layer 0's distinct rows were not counted)
int clip_plan(czc_engine* e, const int* cids, const int* clen, int B, int K, int share, int* totals, PlanBufs* bufs) {
  PlanBufs& p = *bufs;
  E_CHECK(plan_bufs(e, B, K, &p));
  const int S = B + B * K;
  // de-duplication rides on the shared-prefix plan (K > 1 candidates per image; czc_encode_text's independent sequences have none)
  if (!(e->dedup && share && K > 1)) p.rep = nullptr;
  { ProfScope ps(e, "bridge", 0);
    E_CHECK(launch_prefix_plan(cids, clen, B, K, share, p.own_len, p.pre_len, p.src, p.pos0, totals + PT_MAX_LEN, p.img_max, e->st, p.rep,
                               totals + PT_DUP));
    E_CHECK(launch_scan(p.own_len, S, p.own_off, totals, e->st));
    E_CHECK(launch_prefix_finish(p.own_off, p.own_len, B, K, p.pre_off, p.eidx, totals + PT_TRUNK, e->st, p.rep));
    if (e->share_layer0 && share && K > 1 && K <= 1024 && e->fold_ln && e->pack_branches) {  // the tower decides on the sizes whether layer 0 uses it
      E_CHECK(ensure(e, "p_dcount", (size_t)B * 4, (void**)&p.dcount));
      E_CHECK(launch_layer0_count(cids, p.own_len, p.pre_len, B, K, p.dcount, totals + PT_DIST, e->st));
    } }
  E_HIP(hipMemcpyAsync(e->h_totals + HT_PLAN, totals, PLAN_TOTALS, hipMemcpyDeviceToHost, e->st));
  int* flag;
  E_CHECK(ensure(e, "s_nonfinite", 32, (void**)&flag));
  E_HIP(hipMemcpyAsync(e->h_totals + HT_FLAG_PLAN, flag, 4, hipMemcpyDeviceToHost, e->st));  // the previous steps' cosine check
  return 0;
}

// a text tower: its precision and weights, the profile kind of its GEMMs, the workspace name of its features
struct TextTower { int P; std::vector<LayerW>* L; const void* tproj; const char* gk; const char* feat_name; };

// The text tower on a planned set of packed segments: tp.n_seg segments, tp.M rows, tp.n_pool sequences pooled at tp.buf.eidx.
// in_generate: the pass belongs to a czc_generate* step (refine_rows16_now: the refine engine's screening pass on fp16 rows).
int clip_tower_on(czc_engine* e, const TextTower& w, const int* cids, const TowerPlan& tp, float** feat_out, bool in_generate) {
  const czc_config& c = e->cfg;
  const PlanBufs& p = tp.buf;
  const int H = c.clip_hidden, P = w.P, M = tp.M, n_pool = tp.n_pool;
  float *x, *feat, *tok, *pos, *fg, *fb, *pooled = nullptr; void* pa;
  E_CHECK(ensure(e, "c_x", (size_t)M * H * 4, (void**)&x));
  E_CHECK(ensure(e, "c_pa", (size_t)n_pool * H * prec_bytes(P), &pa));
  E_CHECK(ensure(e, w.feat_name, (size_t)n_pool * c.clip_proj * 4, (void**)&feat));
  E_CHECK(need(e, "text_model.embeddings.token_embedding.weight", (size_t)c.clip_vocab * H, &tok));
  E_CHECK(need(e, "text_model.embeddings.position_embedding.weight", (size_t)c.clip_max_pos * H, &pos));
  E_CHECK(need(e, "text_model.final_layer_norm.weight", H, &fg));
  E_CHECK(need(e, "text_model.final_layer_norm.bias", H, &fb));
  const bool r16 = H == 512 && ((e->resid16 >= 1 && P == PREC_BF16) || (e->resid16 >= 2 && P == PREC_F16) ||
                                (P == PREC_F16 && refine_rows16_now(e, in_generate)));
  float* stat0 = nullptr;
  if (r16 && e->fold_ln && !w.L->empty() && (*w.L)[0].qkv_wf) E_CHECK(ensure(e, "c_stat0", (size_t)M * 8 + 256, (void**)&stat0));
  { ProfScope ps(e, "rowops_clip_text", 0);
    E_CHECK(launch_clip_embed(cids, CZC_CLIP_MAX_LEN, p.src, p.pos0, p.own_off, p.own_len, tp.n_seg, tp.max_len, H, tok, pos, x, e->st,
                              r16 ? 1 : 0, stat0, c.clip_eps)); }
  StackDesc d{P, w.L, w.gk, M, H, c.clip_inter, c.clip_heads, c.clip_eps,
              SegTable{p.pre_off, p.pre_len, p.own_off, p.own_len, tp.n_seg, 0, tp.B > 0 ? p.img_max : nullptr}, tp.max_len, 1};
  d.tp = tp; d.pool_idx = p.eidx; d.n_pool = n_pool; d.r16 = r16; d.ln_stat0 = stat0;
  // layer 0 on distinct rows: where the folded path runs under the per-image attention kernel, with 32-bit byte offsets into the
  // compact q/k/v buffer
  if (tp.n_l0 > 0 && tp.n_l0 <= M && e->share_layer0 && stat0 && w.L->size() > 1 && per_image_attention(e, P, tp) &&
      (long)tp.n_l0 * 3 * H * 2 < (1L << 31)) {
    int *rowmap, *dist;
    E_CHECK(ensure(e, "c_l0map", (size_t)M * 4, (void**)&rowmap));
    E_CHECK(ensure(e, "c_l0dist", (size_t)tp.n_l0 * 4, (void**)&dist));
    { ProfScope ps(e, "bridge", 0);
      E_CHECK(launch_layer0_map(cids, p.own_off, p.own_len, p.pre_len, p.dcount, tp.B, tp.K, rowmap, dist, e->st)); }
    d.l0 = Layer0Rows{rowmap, dist, tp.n_l0};
  }
  E_CHECK(clip_stack(e, d, x, &pooled));
  { ProfScope ps(e, "rowops_clip_text", 0);
    const float* src = pooled ? pooled : x; const int* idx = pooled ? nullptr : p.eidx;
    if (r16) E_CHECK(launch_layernorm_x16(P, src, idx, fg, fb, c.clip_eps, n_pool, H, pa, e->st));
    else E_CHECK(launch_layernorm(P, src, idx, fg, fb, c.clip_eps, n_pool, H, pa, nullptr, e->st)); }
  E_CHECK(gemm(e, P, w.gk, pa, H, w.tproj, H, nullptr, nullptr, 0, nullptr, feat, c.clip_proj, n_pool, c.clip_proj, H, ACT_NONE));
  *feat_out = feat;
  return 0;
}

// the engine's text tower on the regular B x K plan built by clip_plan; `exact`: the refine engine's split-fp16 weights
int clip_tower(czc_engine* e, const int* cids, const TowerPlan& tp, float** feat_out, bool in_generate, bool exact = false) {
  const bool x = exact && e->refine;
  return clip_tower_on(e, TextTower{x ? (int)PREC_F16X3 : e->pc, x ? &e->ctext_x : &e->ctext, x ? e->tproj_wx : e->tproj_w,
                                    "gemm_clip_text", "c_feat"}, cids, tp, feat_out, in_generate);
}

constexpr const char* MSG_NONFINITE = "non-finite CLIP cosine: an fp16 quantity overflowed in a tower (fp16 residual rows: set option resid16 = 0 on the bf16 engine, refine_rows16 = 0 on the refine engine; fp16 operands: use CZC_PREC_SPLIT)%s";

// the regular B x K plan clip_plan left in `bufs`, from the totals it read back (after the stream has been synchronised)
// branch_floor: a compact memo step's (StepArgs::branch_floor); 0 everywhere else
int read_totals(czc_engine* e, const PlanBufs& bufs, int B, int K, int branch_floor, TowerPlan* tp) {
  const int* t = e->h_totals + HT_PLAN;
  *tp = TowerPlan{};
  tp->buf = bufs; tp->n_seg = B + B * K; tp->n_pool = B * K; tp->B = B; tp->K = K;
  tp->M = t[PT_ROWS]; tp->max_len = t[PT_MAX_LEN]; tp->max_branch = t[PT_MAX_BRANCH];
  tp->n_l0 = t[PT_DIST] > 0 ? t[PT_TRUNK] + t[PT_DIST] : 0;
  tp->n_dup = t[PT_DUP]; tp->pairs = (double)t[PT_PAIRS];
  // a compacted memo step: a branch longer than 32 rows among the images it skipped would have sent the full batch's launch
  // to the per-segment attention kernel, so it goes there too (round 3: the one batch coupling of the text tower)
  if (branch_floor > 32 && tp->max_branch < branch_floor) tp->max_branch = branch_floor;
  if (e->h_totals[HT_FLAG_PLAN]) return fail(e, CZC_ERR_OVERFLOW, MSG_NONFINITE);
  if (t[PT_OVERFLOW]) return fail(e, CZC_ERR_OVERFLOW, "text bridge overflow (row text > CZC_BRIDGE_MAX_BYTES)%s");
  if (tp->max_len > e->cfg.clip_max_pos || tp->max_len > CZC_CLIP_MAX_LEN) return fail(e, CZC_ERR_ARG, "CLIP sequence longer than max_position_embeddings%s");
  return 0;
}

// plan, size read and tower outside a czc_generate* step (the engine's own rows); *plan (optional): the plan that ran
int clip_text_forward(czc_engine* e, const int* cids, const int* clen, int B, int K, int share, int* totals,
                      float** feat_out, bool exact = false, TowerPlan* plan = nullptr) {
  PlanBufs bufs;
  E_CHECK(clip_plan(e, cids, clen, B, K, share, totals, &bufs));
  E_HIP(hipStreamSynchronize(e->st));  // the one host round trip per step (the reference has one too, gen_utils.py:81)
  TowerPlan tp;
  E_CHECK(read_totals(e, bufs, B, K, 0, &tp));
  E_CHECK(clip_tower(e, cids, tp, feat_out, false, exact));
  e->stat_clip_rows += tp.M;
  e->stat_clip_seqs += B * K;
  if (plan) *plan = tp;
  return 0;
}

// ---- one position-step on the device-resident d_inp (gen_utils.py:66-81), in two halves around the size read ----
// What a step is asked to do beyond its batch.  in_generate: it belongs to a czc_generate* call (czc_step, whose output is all K
// scores, keeps the tighter selection and fp32 rows).  gate: the margin gate is open (czc_generate's steps that are not audited).
// need_cos: the call returns this step's winner cosine, so a gated image re-encodes its winner (read on the gated path only).
struct StepMode { bool in_generate = false, gate = false, need_cos = true; };

// Everything a step reads about its batch and its mode: a caller fills one and a compact batch is a copy with its own rows.
struct StepArgs {
  int* d_inp; int B, T, gen_idx, n_mask, dot_allowed, K;
  czc_hyper hp;
  const float* img = nullptr;  // [B, D] normalised image rows the batch is scored against (the resident batch, a rows call's gather, a compact batch's)
  // czc_generate_rows: column / '.' rule of every row (device, [B]) and the columns' host copy; null = the scalars above
  // (gen_idx then still holds row 0's column: what a control callback is told when all rows share one)
  const int* gen_rows = nullptr; const int* dot_rows = nullptr; const int32_t* gen_rows_host = nullptr;
  // czc_generate_rows_len: the rows' own lengths (T is then the stride of d_inp only); ctl_T: the one length the rows of a step
  // share where a control callback is set -- what it is told as T, with the rows' first ctl_T columns
  const Ragged* rag = nullptr; int ctl_T = 0;
  RowRecords rec;        // the per-row records of these B rows, with the step's index in the call's schedule
  int branch_floor = 0;  // compact memo step: longest branch the images that HIT had (the full batch's attention-kernel choice)
  StepMode mode;
};
struct StepBufs { float *probs, *senti, *reps; int *idxs, *cand, *cids, *clen, *totals; };

int step_bufs(czc_engine* e, int n_seq, StepBufs* b) {
  E_CHECK(ensure(e, "s_probs", (size_t)n_seq * 4, (void**)&b->probs));
  E_CHECK(ensure(e, "s_idxs", (size_t)n_seq * 4, (void**)&b->idxs));
  E_CHECK(ensure(e, "s_cand", (size_t)n_seq * 4, (void**)&b->cand));
  E_CHECK(ensure(e, "s_cids", (size_t)n_seq * CZC_CLIP_MAX_LEN * 4, (void**)&b->cids));
  E_CHECK(ensure(e, "s_clen", (size_t)n_seq * 4, (void**)&b->clen));
  E_CHECK(ensure(e, "s_tot", PLAN_TOTALS, (void**)&b->totals));
  E_CHECK(ensure(e, "s_senti", (size_t)n_seq * 4, (void**)&b->senti));
  E_CHECK(ensure(e, "s_reps", (size_t)n_seq * 4, (void**)&b->reps));
  return 0;
}

// mask -> BERT -> MLM head -> softmax/top-K -> text bridge -> segment plan (*bufs: what it filled) -> start of the size read
int step_phase_a(czc_engine* e, const StepArgs& a, const StepBufs& b, PlanBufs* bufs) {
  const czc_config& c = e->cfg;
  const czc_hyper* hp = &a.hp;
  if (a.n_mask > 0) {
    const bool prune = e->bert_prune && a.n_mask == 1;
    if (a.gen_rows) {
      E_CHECK(launch_mask_positions_rows(a.d_inp, a.B, a.T, a.gen_rows, a.n_mask, c.mask_id, e->st));
      E_CHECK(bert_forward(e, a.d_inp, a.B, a.T, prune ? a.gen_idx : -1, prune ? a.gen_rows : nullptr, a.gen_rows_host, a.rag));
    } else {
      E_CHECK(launch_mask_positions(a.d_inp, a.B, a.T, a.gen_idx, a.n_mask, c.mask_id, e->st));
      E_CHECK(bert_forward(e, a.d_inp, a.B, a.T, prune ? a.gen_idx : -1));
    }
  }
  float* logits;
  E_CHECK(mlm_head(e, a.B, a.T, a.gen_idx, &logits, a.gen_rows, a.gen_rows_host, a.rag));
  { ProfScope ps(e, "topk", 0);
    if (a.rec.vset) E_CHECK(launch_softmax_mask_topk_rows_vocab(logits, a.B, c.bert_vocab, a.K, e->d_mask, a.rec.hp ? a.rec.hp : a.rec.vhp, c.dot_id,
                                                                 a.dot_rows, a.rec.vset, a.rec.vbits, a.rec.vwords, b.probs, b.idxs, b.cand, e->st));
    else if (a.rec.hp) E_CHECK(launch_softmax_mask_topk_rows_hp(logits, a.B, c.bert_vocab, a.K, e->d_mask, a.rec.hp, c.dot_id, a.dot_rows,
                                                             b.probs, b.idxs, b.cand, e->st));
    else if (a.dot_rows) E_CHECK(launch_softmax_mask_topk_rows(logits, a.B, c.bert_vocab, a.K, e->d_mask, hp->temperature, c.dot_id, a.dot_rows,
                                                          b.probs, b.idxs, b.cand, e->st));
    else E_CHECK(launch_softmax_mask_topk(logits, a.B, c.bert_vocab, a.K, e->d_mask, hp->temperature, c.dot_id, a.dot_allowed,
                                          b.probs, b.idxs, b.cand, e->st)); }
  E_HIP(hipMemsetAsync(b.totals, 0, PLAN_TOTALS, e->st));
  { ProfScope ps(e, "bridge", 0);
    PosDev pos{hp->control == 2 ? e->d_pos_tags : nullptr, e->d_pos_masks, e->pos_n};
    // per-row hyper-parameters: every table there is goes along and a candidate's thread scores by its row's control
    if (a.rec.hp) E_CHECK(launch_bridge_rows_hp(e->bd, a.d_inp, a.B, a.T, a.gen_rows, b.cand, a.K, e->d_lex, e->d_lex_pos, e->d_lex_cls, a.rec.hp,
                                                  PosDev{e->d_pos_tags, e->d_pos_masks, e->pos_n}, b.cids, b.clen, b.senti, b.reps,
                                                  b.totals + PT_OVERFLOW, e->st, a.rag ? a.rag->len : nullptr));
    else if (a.gen_rows) E_CHECK(launch_bridge_rows(e->bd, a.d_inp, a.B, a.T, a.gen_rows, b.cand, a.K, hp->control == 1 ? e->d_lex : nullptr,
                                               hp->control == 1 ? e->d_lex_pos : nullptr, e->d_lex_cls, hp->negative,
                                               pos, b.cids, b.clen, b.senti, b.reps, b.totals + PT_OVERFLOW, e->st, a.rag ? a.rag->len : nullptr));
    else E_CHECK(launch_bridge(e->bd, a.d_inp, a.B, a.T, a.gen_idx, b.cand, a.K, hp->control == 1 ? e->d_lex : nullptr,
                               hp->control == 1 ? e->d_lex_pos : nullptr, e->d_lex_cls, hp->negative,
                               pos, b.cids, b.clen, b.senti, b.reps, b.totals + PT_OVERFLOW, e->st)); }
  E_CHECK(clip_plan(e, b.cids, b.clen, a.B, a.K, e->share_prefix, b.totals, bufs));
  return 0;
}

// Control scores from the host (czc_set_control_callback): rows as the reference decodes them at
// control_gen_utils.py:54-57 / :158-160 -- `inp` with [MASK] at gen_idx, candidate k of image b replaces it by cand[b][k].
// The scores are only needed by the combine kernel, so the step fetches the ids with its size read (control_fetch, queued
// in front of the step's one host round trip), launches the CLIP tower, and calls the host WHILE the tower runs
// (control_score): the reference's Python scorer (control_gen_utils.py:56-57) disappears under the tower's GPU time wherever
// it is the shorter of the two.
// a grow-only pinned host buffer: at least `want` bytes behind *p (*cap: what it holds), a quarter more where it has to grow --
// after the stream has drained, since a queued copy may still read the old one
int ensure_pinned(czc_engine* e, int32_t** p, size_t* cap, size_t want) {
  if (*cap >= want) return 0;
  E_HIP(hipStreamSynchronize(e->st));
  if (*p) (void)hipHostFree(*p);
  *p = nullptr; *cap = 0;
  E_HIP(hipHostMalloc((void**)p, want + want / 4));
  *cap = want + want / 4;
  return 0;
}

int control_fetch(czc_engine* e, const StepArgs& a, const StepBufs& b) {
  const int Tc = a.ctl_T > 0 ? a.ctl_T : a.T;
  const size_t n_seq = (size_t)a.B * a.K, n_inp = (size_t)a.B * Tc;
  E_CHECK(ensure_pinned(e, &e->h_ctl_ids, &e->h_ctl_cap, (n_inp + n_seq) * 4 + n_seq * 4));  // [B*T + B*K] ids, [B*K] scores
  e->h_ctl_scores = (float*)(e->h_ctl_ids + n_inp + n_seq);
  if (Tc == a.T) E_HIP(hipMemcpyAsync(e->h_ctl_ids, a.d_inp, n_inp * 4, hipMemcpyDeviceToHost, e->st));
  else E_HIP(hipMemcpy2DAsync(e->h_ctl_ids, (size_t)Tc * 4, a.d_inp, (size_t)a.T * 4, (size_t)Tc * 4, a.B, hipMemcpyDeviceToHost, e->st));
  E_HIP(hipMemcpyAsync(e->h_ctl_ids + n_inp, b.cand, n_seq * 4, hipMemcpyDeviceToHost, e->st));
  return 0;
}

// after the step's host round trip (the ids have landed) and after the tower's launches have been queued
int control_score(czc_engine* e, const StepArgs& a, const StepBufs& b) {
  const int Tc = a.ctl_T > 0 ? a.ctl_T : a.T;
  const size_t n_seq = (size_t)a.B * a.K, n_inp = (size_t)a.B * Tc;
  memset(e->h_ctl_scores, 0, n_seq * 4);
  const int rc = e->ctl_fn(e->ctl_user, e->h_ctl_ids, e->h_ctl_ids + n_inp, a.B, Tc, a.K, a.gen_idx, e->h_ctl_scores);
  if (rc) return fail(e, CZC_ERR_STATE, "the control callback reported an error%s");
  // pinned source: the copy is queued behind the tower; the buffer is next written after the next step's round trip
  E_HIP(hipMemcpyAsync(b.senti, e->h_ctl_scores, n_seq * 4, hipMemcpyHostToDevice, e->st));
  return 0;
}

// CLIP text tower on the planned rows -> cosine / softmax_K / fusion / argmax / write-back; *bcos_out: the winners' cosines [B]
int step_phase_b(czc_engine* e, const StepArgs& a, const StepBufs& b, const TowerPlan& tp, float** bcos_out) {
  const czc_config& c = e->cfg;
  const czc_hyper* hp = &a.hp;
  const int n_seq = a.B * a.K;
  float* feat;
  E_CHECK(clip_tower(e, b.cids, tp, &feat, a.mode.in_generate));
  if (hp->control && e->ctl_fn) E_CHECK(control_score(e, a, b));  // host scorer under the tower that was just queued
  float *cscore, *cref, *fin, *bcos; int* best;
  E_CHECK(ensure(e, "s_cscore", (size_t)n_seq * 4, (void**)&cscore));
  E_CHECK(ensure(e, "s_cref", (size_t)n_seq * 4, (void**)&cref));
  E_CHECK(ensure(e, "s_fin", (size_t)n_seq * 4, (void**)&fin));
  E_CHECK(ensure(e, "s_best", (size_t)a.B * 4, (void**)&best));
  E_CHECK(ensure(e, "s_bcos", (size_t)a.B * 4, (void**)&bcos));
  *bcos_out = bcos;
  CombineArgs ca;
  ca.text_feat = feat; ca.img_n = a.img; ca.logit_scale_exp = e->logit_scale_exp; ca.probs = b.probs; ca.cand = b.cand;
  ca.senti_raw = b.senti; ca.repeats = b.reps; ca.alpha = hp->alpha; ca.beta = hp->beta; ca.gamma = hp->gamma;
  ca.use_senti = hp->control; ca.B = a.B; ca.K = a.K; ca.D = c.clip_proj; ca.clip_score = cscore; ca.clip_ref = cref;
  ca.final_score = fin; ca.best = best; ca.best_cos = bcos; ca.inp = a.d_inp; ca.T = a.T; ca.gen_idx = a.gen_idx;
  ca.hp_rows = a.rec.hp;   // czc_generate_rows_hp: alpha / beta / gamma / control per row, in both passes of the refine engine too
  ca.gen_rows = a.gen_rows;  // both passes of the refine engine write back through the same per-row column
  // czc_generate_rows_draw: the draw belongs to the combine that writes back -- the only one here, the final one of the refine engine
  if (!e->refine) { ca.draw_rows = a.rec.draw; ca.draw_step = a.rec.step; }
  E_CHECK(ensure(e, "s_nonfinite", 32, (void**)&ca.nonfinite));
  if (a.rec.rival) {  // czc_generate_rows_vs (never on the refine engine: refused by the entry point)
    if (e->refine) return fail(e, CZC_ERR_STATE, "step: rivals on the screen-then-refine engine%s");
    ca.rival_idx = a.rec.rival; ca.M = a.rec.M; ca.rival_delta = a.rec.delta; ca.img_all = a.rec.img_all; ca.n_img = a.rec.n_img;
    E_CHECK(ensure(e, "s_disc", (size_t)n_seq * 4, (void**)&ca.disc));
  }
  if (!e->refine) {
    ProfScope ps(e, "combine", 0);
    E_CHECK(launch_combine(ca, e->st));
    return 0;
  }
  // ---- screen-then-refine: scores from the screening cosines (no write-back), selection, second pass, final scores ----
  int *kind, *list, *count, *count_off, *rtot, *rlist;
  float* rcos;
  E_CHECK(ensure(e, "r_kind", (size_t)n_seq * 4, (void**)&kind));
  E_CHECK(ensure(e, "r_list", (size_t)n_seq * 4, (void**)&list));
  E_CHECK(ensure(e, "r_count", (size_t)a.B * 4, (void**)&count));
  E_CHECK(ensure(e, "r_count_off", (size_t)(a.B + 1) * 4, (void**)&count_off));
  E_CHECK(ensure(e, "r_tot", 64, (void**)&rtot));
  E_CHECK(ensure(e, "r_rlist", (size_t)n_seq * 4, (void**)&rlist));
  E_CHECK(ensure(e, "r_cos", (size_t)n_seq * 4, (void**)&rcos));
  const PlanBufs& sp = tp.buf;  // the screening plan
  PlanBufs rp;
  E_CHECK(plan_bufs(e, a.B, a.K, &rp, "r"));
  const int S = a.B + n_seq;
  const bool gen = a.mode.in_generate;
  const float rows16_x = refine_rows16_now(e, gen) ? e->refine_rows16_factor : 1.f;  // what the bounds on the screening deviation grow by on fp16 rows
  const int strata = gen ? e->refine_samples : e->refine_samples_step, need_cos = a.mode.need_cos ? 1 : 0;
  // (on fp16 rows the deviation a kept screening cosine carries is refine_rows16_factor times larger: the mass threshold
  // shrinks by the same factor, so theta * deviation -- what such a candidate can move its score by -- stays what it was)
  const float theta_base = gen ? e->refine_theta_gen / rows16_x : e->refine_theta_x;
  const float theta = theta_base / fmaxf(hp->beta * e->logit_scale_exp, 1e-6f);  // (per-row hyper-parameters: formed per row in the kernel)
  { ProfScope ps(e, "combine", 0);
    ca.inp = nullptr;
    E_CHECK(launch_combine(ca, e->st));
    const float gate_h = a.mode.gate ? e->refine_gate_delta * rows16_x * e->logit_scale_exp : 0.f;
    if (a.rec.draw) E_CHECK(launch_refine_select_draw(cscore, fin, a.B, a.K, theta, theta_base, e->logit_scale_exp, strata, gate_h, hp->beta, a.rec.hp,
                                                      a.rec.draw, need_cos, ca.nonfinite + NF_GATED, kind, list, count, e->st));
    else if (a.rec.hp) E_CHECK(launch_refine_select_rows(cscore, fin, a.B, a.K, theta_base, e->logit_scale_exp, strata, gate_h, a.rec.hp, need_cos,
                                                         ca.nonfinite + NF_GATED, kind, list, count, e->st));
    else E_CHECK(launch_refine_select(cscore, fin, a.B, a.K, theta, strata, gate_h, hp->beta, need_cos, ca.nonfinite + NF_GATED, kind, list, count, e->st)); }
  { ProfScope ps(e, "bridge", 0);
    E_HIP(hipMemsetAsync(rtot, 0, 64, e->st));  // (the buffer's 64 bytes; PLAN_TOTALS of them are read back)
    E_HIP(hipMemsetAsync(rp.own_len, 0, (size_t)S * 4, e->st));
    E_CHECK(launch_scan(count, a.B, count_off, rtot + RT_R, e->st));  // R, then Kr = largest per-image count
    E_CHECK(launch_refine_plan(b.clen, sp.own_len, list, count, count_off, rtot + RT_KR, a.B, a.K, rp.own_len, rp.pre_len, rp.src, rp.pos0,
                               rlist, rtot + PT_MAX_LEN, rp.img_max, e->st));
    E_CHECK(launch_scan(rp.own_len, S, rp.own_off, rtot, e->st));   // rows of the refine pass
    E_CHECK(launch_refine_finish(rp.own_off, rp.own_len, count, count_off, rtot + RT_KR, a.B, a.K, rp.pre_off, rp.eidx, e->st)); }
  E_HIP(hipMemcpyAsync(e->h_totals + HT_REFINE, rtot, PLAN_TOTALS, hipMemcpyDeviceToHost, e->st));
  E_HIP(hipStreamSynchronize(e->st));  // second (and last) host round trip of the step: the sizes of the refine pass
  const int* rt = e->h_totals + HT_REFINE;
  const int M2 = rt[PT_ROWS], R = rt[RT_R], Kr = rt[RT_KR];
  if (R < 0 || R > n_seq || M2 < 0 || Kr < 0 || Kr > a.K) return fail(e, CZC_ERR_STATE, "refine plan returned impossible sizes%s");
  if (R > 0) {
    float* feat2;
    // regular B x Kr plan (empty slots have no rows): the packed-branch split attention serves it like the screening plan
    TowerPlan tp2;
    tp2.buf = rp; tp2.buf.rep = nullptr /* no de-duplication */; tp2.n_seg = a.B + a.B * Kr; tp2.n_pool = R; tp2.B = a.B; tp2.K = Kr;
    tp2.M = M2; tp2.max_len = rt[PT_MAX_LEN]; tp2.max_branch = rt[PT_MAX_BRANCH]; tp2.pairs = (double)rt[PT_PAIRS];
    E_CHECK(clip_tower_on(e, TextTower{PREC_F16X3, &e->ctext_x, e->tproj_wx, "gemm_clip_refine", "c_feat2"}, b.cids, tp2, &feat2, gen));
    ProfScope ps(e, "combine", 0);
    E_CHECK(launch_refine_cosine(feat2, a.img, rlist, count_off + a.B, R, a.K, c.clip_proj, rcos, ca.nonfinite, e->st));
  }
  { ProfScope ps(e, "combine", 0);
    ca.text_feat = nullptr; ca.inp = a.d_inp; ca.refine_kind = kind; ca.refine_cos = rcos;
    ca.draw_rows = a.rec.draw; ca.draw_step = a.rec.step;
    ca.refine_guard = e->refine_guard_dev * rows16_x;
    E_CHECK(launch_combine(ca, e->st)); }
  e->stat_refine_rows += M2;
  e->stat_refine_seqs += R;
  return 0;
}

// The resident image batch as a step's image rows: null (step_device refuses the step) unless it holds exactly B images
const float* resident_images(const czc_engine* e, int B) { return B == e->img_B ? e->d_img_n : nullptr; }

// what a step hands back to callers that read its results on the device: the winners' cosines [B], its plan's longest branch per image [B]
struct StepOut { const float* bcos = nullptr; const int* img_max = nullptr; };

int step_device(czc_engine* e, const StepArgs& a, StepOut* out = nullptr) {
  const czc_config& c = e->cfg;
  const int B = a.B, T = a.T, gen_idx = a.gen_idx, n_mask = a.n_mask, K = a.K;
  const czc_hyper* hp = &a.hp; const Ragged* rag = a.rag;
  if (!e->finalized) return fail(e, CZC_ERR_STATE, "weights not finalized%s");
  if (c.bert_layers <= 0) return fail(e, CZC_ERR_STATE, "this engine was created without the BERT tower%s");
  if (!e->d_mask) return fail(e, CZC_ERR_STATE, "token mask not set%s");
  if (!e->has_bridge) return fail(e, CZC_ERR_STATE, "bridge tables not set%s");
  if (!a.img) return fail(e, CZC_ERR_STATE, "image embeds not set for this batch size%s");
  if (T > CZC_MAX_BERT_LEN || gen_idx < 0 || gen_idx >= T || K > CZC_MAX_TOPK)
    return fail(e, CZC_ERR_ARG, "step: bad T/gen_idx/K%s");
  if (hp->control == 1 && !e->ctl_fn && !e->d_lex && !e->d_lex_pos)
    return fail(e, CZC_ERR_STATE, "sentiment path needs a lexicon (czc_set_lexicon / czc_set_lexicon_pos) or czc_set_control_callback%s");
  if (hp->control == 2 && !e->ctl_fn && !e->d_pos_tags)
    return fail(e, CZC_ERR_STATE, "POS path needs czc_set_pos or czc_set_control_callback%s");
  if (n_mask <= 0 && (e->last_B != B || e->last_T != T))
    return fail(e, CZC_ERR_STATE, "n_mask=0 needs a previous forward of the same [B,T] shape%s");
  if (a.rec.hp && (!a.gen_rows || !a.dot_rows)) return fail(e, CZC_ERR_ARG, "step: per-row hyper-parameters need per-row columns%s");
  if (a.rec.draw && !a.gen_rows) return fail(e, CZC_ERR_ARG, "step: per-row draws need per-row columns%s");
  if (rag && (!a.gen_rows || !a.dot_rows || rag->max_T > T || rag->M > B * T)) return fail(e, CZC_ERR_ARG, "step: ragged rows need per-row columns and lengths within T%s");
  StepBufs b; PlanBufs bufs;
  E_CHECK(step_bufs(e, B * K, &b));
  E_CHECK(step_phase_a(e, a, b, &bufs));
  if (n_mask > 0) { e->stat_bert_rows += rag ? rag->M : B * T; e->last_BT = B * T; e->last_B = B; e->last_T = T; }
  if (hp->control && e->ctl_fn) E_CHECK(control_fetch(e, a, b));  // ids for the host scorer ride on the same round trip
  E_HIP(hipStreamSynchronize(e->st));  // the one host round trip per step (the reference has one too, gen_utils.py:81)
  TowerPlan tp; float* bcos;
  E_CHECK(read_totals(e, bufs, B, K, a.branch_floor, &tp));
  E_CHECK(step_phase_b(e, a, b, tp, &bcos));
  if (out) *out = StepOut{bcos, bufs.img_max};
  e->stat_clip_rows += tp.M;
  e->stat_clip_seqs += B * K;
  e->stat_dedup_seqs += tp.n_dup;
  e->stat_steps += 1;
  return 0;
}

// the end of a call that ran steps, one read: the steps' cosine check, then their guard and gate statistics
int finish_steps(czc_engine* e) {
  int* f = e->h_totals + HT_FLAGS;
  E_HIP(hipMemcpyAsync(f, e->ws["s_nonfinite"].p, NF_READ * 4, hipMemcpyDeviceToHost, e->st));
  E_HIP(hipStreamSynchronize(e->st));
  if (f[NF_NONFINITE]) return fail(e, CZC_ERR_OVERFLOW, MSG_NONFINITE);
  { float dev; memcpy(&dev, f + NF_GUARD_DEV, 4); e->guard_max_dev = fmaxf(e->guard_max_dev, dev); e->guard_trips += f[NF_GUARD_TRIPS];
    e->stat_gated += f[NF_GATED]; e->stat_gate_images += f[NF_GATE_IMAGES]; }
  return CZC_OK;
}

int copy_out(czc_engine* e, void* dst, const char* ws_name, size_t bytes) {
  if (!dst) return 0;
  E_HIP(hipMemcpyAsync(dst, e->ws[ws_name].p, bytes, hipMemcpyDefault, e->st));
  return 0;
}

// Does any option setting of this engine run the text tower on fp16 rows with the LayerNorms folded into its GEMMs?  The folded
// operands (44 MB for 12 layers) are built by czc_finalize_weights only then: the bf16 engine (resid16 >= 1, its default), the
// refine engine whose czc_generate screens on fp16 rows (refine_rows16, default), a single-pass fp16 engine asked for resid16 = 2.
bool wants_folded_ln(const czc_engine* e) {
  if (!prec_is_half(e->pc) || e->cfg.clip_hidden != 512 || !e->fold_ln) return false;
  if (e->pc == PREC_BF16) return e->resid16 >= 1;
  return e->resid16 >= 2 || (e->refine && e->refine_rows16);
}

void free_layer_set(std::vector<LayerW>& L) {
  for (auto& l : L) {
    (void)hipFree(l.qkv_w); (void)hipFree(l.qkv_b); (void)hipFree(l.o_w); (void)hipFree(l.fc1_w); (void)hipFree(l.fc2_w);
    (void)hipFree(l.qkv_wf); (void)hipFree(l.qkv_bf); (void)hipFree(l.fc1_wf); (void)hipFree(l.fc1_bf);
  }
  L.clear();
}

// ---- a generate call as one value --------------------------------------------------------------------------------------
// Every czc_generate* entry point fills a RowsCall and hands it to run_call.  `level` names the entry point and so which optional
// arrays it has; a check_* function validates one array and drops it (null) where it carries nothing, so below them "the call has
// per-row lengths / records / draws / groups / rivals" is a fact of the struct.  A new per-row argument: a field, a check_*
// function, an upload in upload_call and, if kernels read it at every step, a RowRecords entry.
enum CallLevel { CALL_GENERATE, CALL_ROWS, CALL_FROM, CALL_LEN, CALL_HP, CALL_DRAW, CALL_TIED, CALL_VS, CALL_VOCAB };
struct RowsCall {
  CallLevel level = CALL_GENERATE;
  bool rows = false, from = false;  // per-row positions and images / a start row per row and idle positions
  int R = 0, T = 0, L = 0, seed_len = 0, top_k = 0, n_steps = 0, snapshot_every = 0;  // (R: czc_generate's B)
  const int32_t *init = nullptr, *len = nullptr, *image_of_row = nullptr, *group = nullptr, *positions = nullptr, *n_mask = nullptr;
  const czc_hyper *hp = nullptr, *hp_rows = nullptr;  // the call's one record (with per-row records [R]: their entry 0)
  const czc_draw* draw = nullptr;                     // [R]
  const int32_t* rival = nullptr; int M = 0; const float* delta = nullptr;  // [R, M], [R]
  const uint32_t* sets = nullptr; int n_sets = 0; const int32_t* vset = nullptr;  // [n_sets, ceil(bert_vocab / 32)], [R]
  int32_t* out_ids = nullptr; float* out_cos = nullptr;
  std::vector<czc_hyper> vocab_hp;  // upload_call: the R equal records of a vocabulary call whose own were dropped as uniform
  std::vector<czc_draw> no_draw;  // check_rival_table: the tau = 0 records of a rival call that brought none
  size_t n_pos() const { return rows ? (size_t)n_steps * R : (size_t)n_steps; }
  int n_mask_at(int s) const { return n_mask ? n_mask[s] : 1; }
};

// The schedule upload of a rows call (int32 words; the kernels read this layout): [n_steps][R] columns (CZC_POS_IDLE where a row
// sits the step out) | at dot: [n_steps][R] '.' rules | idle calls, at run: [n_steps][R] run lists (every step's rows that are not
// idle, ascending) | len mode, at rag: [R] token counts + [R + 1] packed-row offsets of the full batch, then (idle calls, at
// rag_steps, else 0) one such block per step for its run list
struct SchedLayout {
  int R = 0; bool idle = false;
  size_t dot = 0, run = 0, rag = 0, rag_steps = 0;
  int rag_M = 0, rag_max = 0;  // len mode: packed rows / longest row of the full batch
  size_t rag_block() const { return 2 * (size_t)R + 1; }
  size_t cols(int s) const { return (size_t)s * R; }
  size_t dots(int s) const { return dot + (size_t)s * R; }
  size_t runs(int s) const { return run + (size_t)s * R; }
  size_t rag_step(int s) const { return rag_steps + (size_t)s * rag_block(); }
};
struct Sched { std::vector<int32_t> h; const int* d = nullptr; SchedLayout at; };  // on the host, its upload, where its blocks are

// ---- option "memo" (czc_generate): the step memo of memo.hip ----------------------------------------------------------
// A step group is one n_mask >= 1 step plus the n_mask = 0 steps that re-use its forward (span order: 2 then 0,
// gen_utils.py:160-179).  Its key is the (position, n_mask) list of its steps; an image's entry at that key holds the masked
// row of the group's first step (which fixes the outcome of every step of the group), the row and winner cosine each step
// left, and each step's longest CLIP branch.  Entries live for one call.
constexpr int MEMO_SUB = 2;  // steps per group the entry has room for (a longer group runs without the memo)

// The step groups of a call's schedule, shared by the step memo and the rows memo (n_mask is one value per step for all rows)
struct StepGroups {
  std::vector<int> first, sub, len;  // per step: first step of its group, index inside the group; per group-start step: its steps
  // per group-start step: the group may take an entry back.  CZC_PREC_REFINE: not where a step is audited (the guard stays on every
  // image) or returns its winner cosine (a split re-encode whose last bits can depend on which other candidates went with the winner)
  std::vector<char> hittable;
};

StepGroups step_groups(const czc_engine* e, const RowsCall& c, const std::vector<char>& audit) {
  const int n_steps = c.n_steps;
  StepGroups G;
  G.first.assign(n_steps, 0); G.sub.assign(n_steps, 0); G.len.assign(n_steps, 0); G.hittable.assign(n_steps, 0);
  for (int s = 0; s < n_steps; s += G.len[s]) {
    int g = 1;
    while (s + g < n_steps && c.n_mask && c.n_mask[s + g] <= 0) ++g;
    G.len[s] = g;
    G.hittable[s] = 1;
    for (int j = 0; j < g; ++j) {
      G.first[s + j] = s; G.sub[s + j] = j;
      const bool cos_out = c.out_cos && (s + j + 1) % c.snapshot_every == 0;
      if (e->refine && (audit[s + j] || cos_out)) G.hittable[s] = 0;
    }
  }
  return G;
}

struct MemoPlan {
  StepGroups grp;
  std::vector<int> slot;       // per step: entry slot of its group (-1: never memoised)
  std::vector<char> check;     // per group-start step: the host knows the key was visited before and the step may hit
  int *key = nullptr, *rows = nullptr, *imax = nullptr, *hit = nullptr, *list = nullptr, *tot = nullptr, *inp_c = nullptr;
  float *cos = nullptr, *bcos = nullptr, *img_c = nullptr;
  int n_act = 0;  // of the group in progress
  int branch_max[MEMO_SUB] = {0, 0};
};

int memo_begin(czc_engine* e, const RowsCall& c, const std::vector<char>& audit, MemoPlan* mp) {
  const int B = c.R, T = c.T, n_steps = c.n_steps;
  mp->grp = step_groups(e, c, audit);
  mp->slot.assign(n_steps, -1); mp->check.assign(n_steps, 0);
  std::map<std::vector<int>, int> slots;
  for (int s = 0; s < n_steps; s += mp->grp.len[s]) {
    const int g = mp->grp.len[s];
    if (c.n_mask_at(s) < 1 || g > MEMO_SUB) continue;
    std::vector<int> key;
    for (int j = 0; j < g; ++j) { key.push_back(c.positions[s + j]); key.push_back(c.n_mask_at(s + j)); }
    auto it = slots.find(key);
    const bool seen = it != slots.end();
    const int sl = seen ? it->second : (int)slots.size();
    if (!seen) slots[key] = sl;
    for (int j = 0; j < g; ++j) mp->slot[s + j] = sl;
    mp->check[s] = seen && mp->grp.hittable[s];
  }
  const size_t n_slots = slots.size() ? slots.size() : 1, D = (size_t)e->cfg.clip_proj;
  E_CHECK(ensure(e, "m_key", n_slots * B * T * 4, (void**)&mp->key));
  E_CHECK(ensure(e, "m_rows", n_slots * MEMO_SUB * B * T * 4, (void**)&mp->rows));
  E_CHECK(ensure(e, "m_cos", n_slots * MEMO_SUB * B * 4, (void**)&mp->cos));
  E_CHECK(ensure(e, "m_imax", n_slots * MEMO_SUB * B * 4, (void**)&mp->imax));
  E_CHECK(ensure(e, "m_hit", (size_t)B * 4, (void**)&mp->hit));
  E_CHECK(ensure(e, "m_list", (size_t)B * 4, (void**)&mp->list));
  E_CHECK(ensure(e, "m_tot", 16, (void**)&mp->tot));
  E_CHECK(ensure(e, "m_bcos", (size_t)B * 4, (void**)&mp->bcos));
  E_CHECK(ensure(e, "m_inp_c", (size_t)B * T * 4, (void**)&mp->inp_c));
  E_CHECK(ensure(e, "m_img_c", (size_t)B * D * 4, (void**)&mp->img_c));
  return 0;
}

// One step of czc_generate with the memo on (full: the step on the whole batch, as it runs without the memo).  First step of a
// group whose key this call has seen: the check kernel and one 16-byte read (the second host round trip of such a step) give the
// active images; then all of them run as usual (and record), none of them runs (BERT, the towers and the combine kernel are
// skipped), or the step runs on a compact batch of them: a copy of `full` with its own rows and image rows.  The group's other
// steps keep its active set: the n_mask = 0 step re-uses the forward of exactly those rows.
int memo_step(czc_engine* e, MemoPlan& mp, int s, const StepArgs& full) {
  int* const d_inp = full.d_inp;
  const int B = full.B, T = full.T, gen_idx = full.gen_idx, n_mask = full.n_mask;
  const int slot = mp.slot[s], j = mp.grp.sub[s], mask_id = e->cfg.mask_id, D = e->cfg.clip_proj;
  int* key = slot >= 0 ? mp.key + (size_t)slot * B * T : nullptr;
  int* rows = slot >= 0 ? mp.rows + ((size_t)slot * MEMO_SUB + j) * B * T : nullptr;
  float* cos = slot >= 0 ? mp.cos + ((size_t)slot * MEMO_SUB + j) * B : nullptr;
  int* imax = slot >= 0 ? mp.imax + ((size_t)slot * MEMO_SUB + j) * B : nullptr;
  if (j == 0) {
    mp.n_act = B;
    mp.branch_max[0] = mp.branch_max[1] = 0;
    if (mp.check[s]) {
      E_CHECK(launch_memo_check(d_inp, B, T, gen_idx, n_mask, mask_id, key, mp.imax + (size_t)slot * MEMO_SUB * B, mp.grp.len[s],
                                mp.hit, mp.list, mp.tot, e->st));
      E_HIP(hipMemcpyAsync(e->h_totals + HT_MEMO, mp.tot, 16, hipMemcpyDeviceToHost, e->st));
      E_HIP(hipStreamSynchronize(e->st));
      mp.n_act = e->h_totals[HT_MEMO + MC_ACTIVE];
      mp.branch_max[0] = e->h_totals[HT_MEMO + MC_BRANCH0]; mp.branch_max[1] = e->h_totals[HT_MEMO + MC_BRANCH1];
      if (mp.n_act < 0 || mp.n_act > B) return fail(e, CZC_ERR_STATE, "memo check returned an impossible count%s");
      // the split-fp16 text tower picks its GEMM forms (split-K slices, ring / tiled kernels) by row count, so a compact batch
      // moves its cosines in the last bits: that engine skips the steps every image hits and runs the others whole
      if (e->pc == PREC_F16X3 && mp.n_act > 0) mp.n_act = B;
    }
  }
  const int n_act = mp.n_act;
  e->stat_memo_images += B;
  e->stat_memo_hits += B - n_act;
  if (n_act < B) E_CHECK(launch_memo_fill(mp.hit, B, T, rows, cos, d_inp, mp.bcos, e->st));
  if (n_act == 0) return 0;
  const bool whole = n_act == B;
  StepArgs a = full;
  if (whole) {  // the whole batch, in place, as without the memo; then the entry is recorded
    if (key && j == 0) E_CHECK(launch_memo_gather(d_inp, nullptr, B, T, gen_idx, n_mask, mask_id, key, nullptr, nullptr, D, nullptr, e->st));
  } else {  // compact batch: rows and normalised image embeds of the active images, the step on them, then their rows and cosines
            // back into the full batch and into the entry
    E_CHECK(launch_memo_gather(d_inp, mp.list, n_act, T, gen_idx, n_mask, mask_id, j == 0 ? key : nullptr, mp.inp_c, full.img, D,
                               mp.img_c, e->st));
    a.d_inp = mp.inp_c; a.B = n_act; a.img = mp.img_c; a.branch_floor = mp.branch_max[j];
  }
  StepOut so;
  E_CHECK(step_device(e, a, &so));
  return launch_memo_scatter(a.d_inp, so.bcos, so.img_max, whole ? nullptr : mp.list, n_act, T,
                             d_inp, mp.bcos, rows, cos, imax, e->st) ? fail(e, CZC_ERR_HIP, "%s", g_err) : 0;
}

// ---- option "memo_rows" (czc_generate_rows): the per-row step memo of memo_rows.hip -----------------------------------
// n_mask is one value per step for all rows, so the step groups are the step memo's (StepGroups) and shared by the rows; the positions
// are per row.  Row r's entry for a group sits in slot (first position of the group, r) under the group's signature (n_mask,
// length, column of the second step): the same first position under another shape replaces it.
struct MemoRowsPlan {
  StepGroups grp;
  std::vector<char> record;      // per group-start step: the group has an entry (starts with n_mask >= 1, fits MEMO_ROWS_SUB)
  std::vector<char> check;       // per group-start step: the host knows some row revisits a key and the step may hit
  MemoRowsTab tab{};
  int *hit = nullptr, *cnt = nullptr, *list = nullptr, *tot = nullptr, *inp_c = nullptr, *col_c = nullptr, *dot_c = nullptr;
  float *bcos = nullptr, *img_c = nullptr;
  // room for the RowRecords of a compact batch's rows, gathered by its run list (a record the call does not carry has none)
  struct { RowHyper* hp = nullptr; RowDraw* draw = nullptr; int* rival = nullptr; float* delta = nullptr; int* vset = nullptr; } rec_c;
  std::vector<std::vector<int32_t>> h_col_c;  // compact batch of the group in progress: the active rows' column at every step
  std::vector<int32_t> run_h;    // of the group in progress: the rows that run, ascending (host copy of list_d)
  const int* list_d = nullptr;   // of the group in progress: the device list of the rows that run (null: every row)
  bool table = false;            // the entries exist (option "memo_rows"); false: the plan only compacts idle rows away
  int n_run = 0;  // of the group in progress: rows that are not idle
  int n_act = 0;  // of the group in progress: rows that run (not idle and no hit)
  int branch_max[MEMO_ROWS_SUB] = {0, 0};
  // czc_generate_rows_len (len_h null otherwise): every row's token count T_r on the host; the offsets / lengths of every step's
  // run list are in the schedule upload (SchedLayout: rag_steps); d_rag_c [2 R + 1]: those of a checked step's compact batch,
  // uploaded after the list read
  const int32_t* len_h = nullptr;
  int* d_rag_c = nullptr;
  Ragged rag_c{};  // of the group in progress, where it runs on a compact batch
  int ctl_T() const { return len_h && !run_h.empty() ? len_h[run_h[0]] : 0; }
};

// the signature word of memo_rows.hip (mr_sig) as the host keeps it to tell whether a step can hit at all
static inline int memo_rows_sig(int n_mask0, int n_sub, int col1) { return (n_mask0 & 0xff) | (n_sub << 8) | ((n_sub > 1 ? col1 + 1 : 0) << 16); }

// table = false (czc_generate_rows_from with idle steps, option off): no entries, nothing is recorded or checked; the plan
// then only carries the compact-batch buffers and the full-batch cosines.  Idle rows (position CZC_POS_IDLE) visit no key.
int memo_rows_begin(czc_engine* e, const RowsCall& c, const std::vector<char>& audit, MemoRowsPlan* mp) {
  const int R = c.R, T = c.T, L = c.L, seed_len = c.seed_len, n_steps = c.n_steps;
  const int32_t* positions = c.positions;
  const czc_draw* draw_host = c.draw;
  const bool table = e->memo_rows;
  static_assert(MEMO_ROWS_SUB == MEMO_SUB, "the rows memo keeps the step memo's group size");
  mp->grp = step_groups(e, c, audit);
  mp->record.assign(n_steps, 0); mp->check.assign(n_steps, 0);
  mp->table = table;
  std::vector<int> seen(table ? (size_t)R * L : 0, -1);  // per slot: the signature it was last recorded under in this call
  for (int s = 0; table && s < n_steps; s += mp->grp.len[s]) {
    const int g = mp->grp.len[s], nm0 = c.n_mask_at(s);
    if (nm0 < 1 || nm0 > T || g > MEMO_ROWS_SUB) continue;
    bool revisit = false;
    for (int r = 0; r < R; ++r) {
      if (positions[(size_t)s * R + r] < 0) continue;  // idle: not a visit
      if (draw_host && draw_host[r].tau > 0.f) continue;  // a row that draws never hits (the check kernel refuses it too)
      const int sig = memo_rows_sig(nm0, g, g > 1 ? seed_len + positions[(size_t)(s + 1) * R + r] : 0);
      int& was = seen[(size_t)r * L + positions[(size_t)s * R + r]];
      revisit = revisit || was == sig;
      was = sig;
    }
    mp->record[s] = 1;
    mp->check[s] = revisit && mp->grp.hittable[s];
  }
  MemoRowsTab& m = mp->tab;
  m.R = R; m.T = T; m.L = L; m.seed_len = seed_len;
  const size_t n_slot = (size_t)L * R, D = (size_t)e->cfg.clip_proj;
  if (table) {
    E_CHECK(ensure(e, "mr_valid", n_slot * 4, (void**)&m.valid));
    E_CHECK(ensure(e, "mr_sig", n_slot * 4, (void**)&m.sig));
    E_CHECK(ensure(e, "mr_key", n_slot * T * 4, (void**)&m.key));
    E_CHECK(ensure(e, "mr_rows", n_slot * MEMO_ROWS_SUB * T * 4, (void**)&m.rows));
    E_CHECK(ensure(e, "mr_cos", n_slot * MEMO_ROWS_SUB * 4, (void**)&m.cos));
    E_CHECK(ensure(e, "mr_imax", n_slot * MEMO_ROWS_SUB * 4, (void**)&m.imax));
    E_CHECK(ensure(e, "mr_hit", (size_t)R * 4, (void**)&mp->hit));
    E_CHECK(ensure(e, "mr_cnt", (size_t)((R + 255) / 256) * 4, (void**)&mp->cnt));
    E_CHECK(ensure(e, "mr_list", (size_t)R * 4, (void**)&mp->list));
    E_CHECK(ensure(e, "mr_tot", 16, (void**)&mp->tot));
  }
  E_CHECK(ensure(e, "mr_bcos", (size_t)R * 4, (void**)&mp->bcos));
  E_CHECK(ensure(e, "mr_inp_c", (size_t)R * T * 4, (void**)&mp->inp_c));
  E_CHECK(ensure(e, "mr_img_c", (size_t)R * D * 4, (void**)&mp->img_c));
  E_CHECK(ensure(e, "mr_col_c", (size_t)R * 4, (void**)&mp->col_c));
  E_CHECK(ensure(e, "mr_dot_c", (size_t)R * 4, (void**)&mp->dot_c));
  if (!table) return 0;
  E_HIP(hipMemsetAsync(m.valid, 0, n_slot * 4, e->st));  // entries live for one call
  // the check's totals (16 bytes), then its list; then (len mode) the compact batch's lengths and offsets
  return ensure_pinned(e, &e->h_memo_list, &e->h_memo_list_cap, ((size_t)R + 4 + 2 * (size_t)R + 1) * 4);
}

// The records of the rows a compact batch runs on: the full batch's, each gathered by the run list the batch is gathered with into
// the plan's compact set
int memo_rows_records(czc_engine* e, const MemoRowsPlan& mp, const RowRecords& full, int n_act, RowRecords* out) {
  *out = full;
  if (full.hp) {
    if (!mp.rec_c.hp || !mp.list_d) return fail(e, CZC_ERR_STATE, "generate_rows_hp: a compact batch without room for its hyper-parameters%s");
    E_CHECK(launch_gather_row_hyper(full.hp, mp.list_d, n_act, mp.rec_c.hp, e->st));
    out->hp = mp.rec_c.hp;
  }
  if (full.draw) {
    if (!mp.rec_c.draw || !mp.list_d) return fail(e, CZC_ERR_STATE, "generate_rows_draw: a compact batch without room for its draw records%s");
    E_CHECK(launch_gather_row_draw(full.draw, mp.list_d, n_act, mp.rec_c.draw, e->st));
    out->draw = mp.rec_c.draw;
  }
  if (full.rival) {
    if (!mp.rec_c.rival || !mp.rec_c.delta || !mp.list_d) return fail(e, CZC_ERR_STATE, "generate_rows_vs: a compact batch without room for its rival tables%s");
    E_CHECK(launch_gather_rows_w32(full.rival, mp.list_d, n_act, full.M, mp.rec_c.rival, e->st));
    E_CHECK(launch_gather_rows_w32(full.delta, mp.list_d, n_act, 1, mp.rec_c.delta, e->st));
    out->rival = mp.rec_c.rival; out->delta = mp.rec_c.delta;
  }
  if (full.vset) {  // (the bitsets stay where they are, like img_all)
    if (!mp.rec_c.vset || !mp.list_d) return fail(e, CZC_ERR_STATE, "generate_rows_vocab: a compact batch without room for its set indices%s");
    E_CHECK(launch_gather_rows_w32(full.vset, mp.list_d, n_act, 1, mp.rec_c.vset, e->st));
    out->vset = mp.rec_c.vset;
  }
  return 0;
}

// One step of czc_generate_rows with the rows memo on, and of czc_generate_rows_from wherever a call has idle steps (with the
// option or without: mp.table); sc: the call's schedule (SchedLayout), full: the step on all R rows.  A row is idle for a whole
// group or for none of it (checked by the caller), so the group's first step decides who runs: the rows that are not idle and,
// where the check ran, did not hit.  First step of a group in which some row revisits a key: the check kernels and one read (totals
// and the ascending active list) give the active rows; then all of them run as without the option (and record), none runs, or the
// step runs on a compact batch whose column / '.' arrays the gather kernel builds.  The compact columns' host copy keeps the
// per-row n_mask = 0 re-use rule of mlm_head in force.
int memo_rows_step(czc_engine* e, MemoRowsPlan& mp, const RowsCall& c, const Sched& sc, int s, const StepArgs& full) {
  int* const d_inp = full.d_inp;
  const int R = c.R, L = c.L, seed_len = c.seed_len;
  const int s0 = mp.grp.first[s], j = mp.grp.sub[s], g = mp.grp.len[s0], mask_id = e->cfg.mask_id, D = e->cfg.clip_proj;
  const int n_mask0 = c.n_mask_at(s0), record = mp.record[s0];
  const int32_t* sched = sc.h.data();
  const int* col0 = sc.d + sc.at.cols(s0);
  const int* col1 = g > 1 ? sc.d + sc.at.cols(s0 + 1) : nullptr;
  const int* col = sc.d + sc.at.cols(s);
  const int* dot = sc.d + sc.at.dots(s);
  if (j == 0) {
    mp.run_h.clear();
    for (int r = 0; r < R; ++r)
      if (sched[(size_t)s0 * R + r] >= 0) mp.run_h.push_back(r);
    mp.n_run = mp.n_act = (int)mp.run_h.size();
    mp.list_d = mp.n_run < R ? sc.d + sc.at.runs(s0) : nullptr;  // the schedule's own run list of this step
    mp.branch_max[0] = mp.branch_max[1] = 0;
    if (mp.check[s]) {
      E_CHECK(launch_memo_rows_check(d_inp, mp.tab, col0, col1, n_mask0, g, mask_id, mp.hit, mp.cnt, mp.list, mp.tot, e->st, full.rec.draw));
      int32_t* h = e->h_memo_list;
      E_HIP(hipMemcpyAsync(h, mp.tot, 16, hipMemcpyDeviceToHost, e->st));
      E_HIP(hipMemcpyAsync(h + 4, mp.list, (size_t)R * 4, hipMemcpyDeviceToHost, e->st));
      E_HIP(hipStreamSynchronize(e->st));
      mp.n_act = h[0];
      mp.branch_max[0] = h[1]; mp.branch_max[1] = h[2];
      if (mp.n_act < 0 || mp.n_act > mp.n_run) return fail(e, CZC_ERR_STATE, "memo_rows check returned an impossible count%s");
      // CZC_PREC_SPLIT: a compact batch moves its cosines in the last bits (memo_step), so a step runs whole -- on every row
      // that is not idle, which is what it runs on with the option off -- unless every such row hits
      if (e->pc == PREC_F16X3 && mp.n_act > 0) mp.n_act = mp.n_run;
      else if (mp.n_act > 0 && mp.n_act < R) {
        mp.list_d = mp.list;
        mp.run_h.resize(mp.n_act);
        for (int i = 0; i < mp.n_act; ++i) {
          const int r = h[4 + i];
          if (r < 0 || r >= R || (i > 0 && r <= h[4 + i - 1]) || sched[(size_t)s0 * R + r] < 0)
            return fail(e, CZC_ERR_STATE, "memo_rows check returned an impossible list%s");
          mp.run_h[i] = r;
        }
      }
    }
    if (mp.n_act > 0 && mp.n_act < R) {
      mp.h_col_c.resize(g);
      for (int jj = 0; jj < g; ++jj) {
        mp.h_col_c[jj].resize(mp.n_act);
        for (int i = 0; i < mp.n_act; ++i) mp.h_col_c[jj][i] = sched[(size_t)(s0 + jj) * R + mp.run_h[i]];
      }
      if (mp.len_h) {  // the compact batch's packed rows: the schedule's own for a run list, built here for a checked step's list
        const bool own = mp.list_d == mp.list;
        if (!own && !sc.at.rag_steps) return fail(e, CZC_ERR_STATE, "generate_rows_len: a run list without its offsets%s");
        int32_t* h = own ? e->h_memo_list + 4 + R : nullptr;  // pinned; the previous upload from it was queued in front of this step's list read
        int M = 0, mx = 0;
        for (int i = 0; i < mp.n_act; ++i) {
          const int t = mp.len_h[mp.run_h[i]];
          if (own) { h[i] = t; h[R + i] = M; }
          M += t; mx = t > mx ? t : mx;
        }
        if (own) {
          h[R + mp.n_act] = M;
          E_HIP(hipMemcpyAsync(mp.d_rag_c, h, ((size_t)2 * R + 1) * 4, hipMemcpyHostToDevice, e->st));
        }
        const int* base = own ? mp.d_rag_c : sc.d + sc.at.rag_step(s0);
        mp.rag_c = Ragged{base + R, base, M, mx};
      }
    }
  }
  const int n_act = mp.n_act;
  if (mp.table) {  // an idle row-step is not a visit: neither counted nor a hit
    e->stat_memo_row_steps += mp.n_run;
    e->stat_memo_row_hits += mp.n_run - n_act;
  }
  if (n_act < mp.n_run) E_CHECK(launch_memo_rows_fill(mp.hit, mp.tab, col0, j, d_inp, mp.bcos, e->st));  // only after a check
  if (n_act == 0) return 0;  // every row idle or hit: nothing runs
  const bool whole = n_act == R;
  StepArgs a = full;
  if (whole) {  // every row, in place, as without the option; then the entries are recorded
    if (record && j == 0)
      E_CHECK(launch_memo_rows_gather(d_inp, nullptr, R, mp.tab, col0, col1, n_mask0, g, mask_id, 1, col, dot, nullptr, nullptr, D,
                                      nullptr, nullptr, nullptr, e->st));
  } else {  // compact batch: rows, row-gathered image embeds, columns, '.' rules and records of the active rows, the step on them,
            // then their rows and cosines back into the batch and into their own slots
    E_CHECK(launch_memo_rows_gather(d_inp, mp.list_d, n_act, mp.tab, col0, col1, n_mask0, g, mask_id, record && j == 0 ? 1 : 0, col, dot,
                                    mp.inp_c, full.img, D, mp.img_c, mp.col_c, mp.dot_c, e->st));
    const int32_t* col_h = mp.h_col_c[j].data();
    a.d_inp = mp.inp_c; a.B = n_act; a.img = mp.img_c;
    a.gen_idx = col_h[0]; a.dot_allowed = col_h[0] - seed_len == L - 1 ? 1 : 0;
    a.gen_rows = mp.col_c; a.dot_rows = mp.dot_c; a.gen_rows_host = col_h; a.rag = mp.len_h ? &mp.rag_c : nullptr; a.ctl_T = mp.ctl_T();
    a.branch_floor = j < MEMO_ROWS_SUB ? mp.branch_max[j] : 0;
    E_CHECK(memo_rows_records(e, mp, full.rec, n_act, &a.rec));
  }
  StepOut so;
  E_CHECK(step_device(e, a, &so));
  return launch_memo_rows_scatter(a.d_inp, so.bcos, so.img_max, whole ? nullptr : mp.list_d,
                                  n_act, mp.tab, col0, j, record, d_inp, mp.bcos, e->st) ? fail(e, CZC_ERR_HIP, "%s", g_err) : 0;
}

// czc_score_rows on the device: CLIP cosine of rows [n, T] (BERT ids; len: the rows' token counts or null = T) with
// img_rows [n, D] (normalised, row-gathered) -> cos [n].  The text bridge on the row itself -- the per-row form with K = 1 and
// a candidate that repeats the id column 0 holds -- then the tower as czc_encode_text runs it (independent sequences, the
// exact tower of the engine precision) and the steps' cosine kernel.  Buffers of its own: a step's are left alone.
// d_rival [n, M] (czc_score_rows_vs; null otherwise): indices into the resident batch (e->d_img_n); the rival cosine kernel then leaves the same
// cosines and d_disc [n] = P(own image | row) among the row's own image and its rivals
int score_rows_device(czc_engine* e, const int* d_rows, int n, int T, const int* d_len, const float* img_rows, float* d_cos,
                      const int* d_rival = nullptr, int M = 0, float* d_disc = nullptr) {
  if (!e->finalized) return fail(e, CZC_ERR_STATE, "weights not finalized%s");
  if (!e->has_bridge) return fail(e, CZC_ERR_STATE, "bridge tables not set%s");
  int *gen, *cand, *cids, *clen, *totals, *flag;
  E_CHECK(ensure(e, "sc_gen", (size_t)n * 4, (void**)&gen));
  E_CHECK(ensure(e, "sc_cand", (size_t)n * 4, (void**)&cand));
  E_CHECK(ensure(e, "sc_cids", (size_t)n * CZC_CLIP_MAX_LEN * 4, (void**)&cids));
  E_CHECK(ensure(e, "sc_clen", (size_t)n * 4, (void**)&clen));
  E_CHECK(ensure(e, "sc_tot", PLAN_TOTALS, (void**)&totals));
  E_CHECK(ensure(e, "s_nonfinite", 32, (void**)&flag));
  E_HIP(hipMemsetAsync(gen, 0, (size_t)n * 4, e->st));
  E_HIP(hipMemsetAsync(totals, 0, PLAN_TOTALS, e->st));
  E_HIP(hipMemcpy2DAsync(cand, 4, d_rows, (size_t)T * 4, 4, n, hipMemcpyDeviceToDevice, e->st));  // column 0 of every row
  { ProfScope ps(e, "bridge", 0);
    E_CHECK(launch_bridge_rows(e->bd, d_rows, n, T, gen, cand, 1, nullptr, nullptr, e->d_lex_cls, 0, PosDev{nullptr, nullptr, 0}, cids, clen,
                               nullptr, nullptr, totals + PT_OVERFLOW, e->st, d_len)); }
  float* feat;
  E_CHECK(clip_text_forward(e, cids, clen, n, 1, 0, totals, &feat, true));  // exact tower; (reads the bridge's overflow flag with the sizes)
  { ProfScope ps(e, "combine", 0);
    if (d_rival) E_CHECK(launch_cosine_rival(feat, img_rows, n, 1, e->cfg.clip_proj, d_rival, M, e->d_img_n, e->img_B, e->logit_scale_exp, d_cos,
                                             d_disc, flag, e->st));
    else E_CHECK(launch_cosine(feat, img_rows, n, 1, e->cfg.clip_proj, d_cos, flag, e->st)); }
  return 0;
}

// czc_generate_rows_tied: the group table of a call.  Host: dense group of every row, members (CSR, ascending, so a group's
// first member is its lowest-numbered row).  Device (one upload): [R] group of row | [G + 1] offsets | [R] members |
// [G] leaders | [G] the leaders' token counts (len mode; else unused)
struct TiePlan {
  int G = 0;
  std::vector<int32_t> host;
  int *d_gor = nullptr, *d_off = nullptr, *d_rows = nullptr, *d_lead = nullptr, *d_lead_len = nullptr;
  int* rows_c = nullptr; float *img_c = nullptr, *cos_c = nullptr, *cos = nullptr;
};

int tie_begin(czc_engine* e, int R, int T, int seed_len, const int32_t* group, const int32_t* len_rows, bool want_cos, TiePlan* tp) {
  std::vector<int32_t> dense(R, -1), gor(R);
  int G = 0;
  for (int r = 0; r < R; ++r) { if (dense[group[r]] < 0) dense[group[r]] = G++; gor[r] = dense[group[r]]; }
  tp->G = G;
  std::vector<int32_t>& h = tp->host;
  h.assign((size_t)2 * R + 3 * G + 1, 0);
  int32_t *off = h.data() + R, *rows = off + G + 1, *lead = rows + R, *lead_len = lead + G;
  for (int r = 0; r < R; ++r) { h[r] = gor[r]; ++off[gor[r] + 1]; }
  for (int g = 0; g < G; ++g) off[g + 1] += off[g];
  std::vector<int32_t> fill(off, off + G);
  for (int r = 0; r < R; ++r) rows[fill[gor[r]]++] = r;
  for (int g = 0; g < G; ++g) { lead[g] = rows[off[g]]; lead_len[g] = len_rows ? seed_len + len_rows[lead[g]] + 1 : T; }
  int* d;
  E_CHECK(ensure(e, "g_tie", h.size() * 4, (void**)&d));
  E_HIP(hipMemcpyAsync(d, h.data(), h.size() * 4, hipMemcpyHostToDevice, e->st));
  tp->d_gor = d; tp->d_off = d + R; tp->d_rows = tp->d_off + G + 1; tp->d_lead = tp->d_rows + R; tp->d_lead_len = tp->d_lead + G;
  if (want_cos) {
    E_CHECK(ensure(e, "t_rows_c", (size_t)G * T * 4, (void**)&tp->rows_c));
    E_CHECK(ensure(e, "t_img_c", (size_t)G * e->cfg.clip_proj * 4, (void**)&tp->img_c));
    E_CHECK(ensure(e, "t_cos_c", (size_t)G * 4, (void**)&tp->cos_c));
    E_CHECK(ensure(e, "t_cos", (size_t)R * 4, (void**)&tp->cos));
  }
  return 0;
}

// the merged captions' cosines at a snapshot: one row per group (its leader) through score_rows_device, then to every member
// img_rows [R, D]: the call's image rows (CallBatch::img)
int tie_score(czc_engine* e, const TiePlan& tp, const int* d_inp, const float* img_rows, int R, int T, bool len_mode) {
  const int D = e->cfg.clip_proj;
  E_CHECK(launch_gather_rows_w32(d_inp, tp.d_lead, tp.G, T, tp.rows_c, e->st));
  E_CHECK(launch_gather_rows_f32(img_rows, tp.d_lead, tp.G, D, tp.img_c, e->st));
  E_CHECK(score_rows_device(e, tp.rows_c, tp.G, T, len_mode ? tp.d_lead_len : nullptr, tp.img_c, tp.cos_c));
  E_CHECK(launch_gather_rows_w32(tp.cos_c, tp.d_gor, R, 1, tp.cos, e->st));
  return 0;
}

}  // namespace

// =================================================================================================
extern "C" {

int czc_version(void) { return 108; }

const char* czc_last_error(const czc_engine* e) { return e ? e->err : czc::g_err; }

int czc_create(const czc_config* cfg, int device_id, czc_engine** out) {
  if (!cfg || !out) { snprintf(czc::g_err, sizeof(czc::g_err), "czc_create: null argument"); return CZC_ERR_ARG; }
  if (cfg->bert_hidden != cfg->bert_heads * 64 || cfg->clip_hidden != cfg->clip_heads * 64 ||
      cfg->vis_hidden != cfg->vis_heads * 64) {
    snprintf(czc::g_err, sizeof(czc::g_err), "czc_create: head_dim must be 64 for all towers");
    return CZC_ERR_ARG;
  }
  if (cfg->precision != CZC_PREC_BF16 && cfg->precision != CZC_PREC_F32 && cfg->precision != CZC_PREC_ALL_BF16 &&
      cfg->precision != CZC_PREC_SPLIT && cfg->precision != CZC_PREC_FP16 && cfg->precision != CZC_PREC_REFINE) {
    snprintf(czc::g_err, sizeof(czc::g_err), "czc_create: unknown precision");
    return CZC_ERR_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    snprintf(czc::g_err, sizeof(czc::g_err), "czc_create: no HIP device visible (the engine has no CPU fallback)");
    return CZC_ERR_HIP;
  }
  if (device_id < 0 || device_id >= ndev) {
    snprintf(czc::g_err, sizeof(czc::g_err), "czc_create: device %d out of range", device_id);
    return CZC_ERR_ARG;
  }
  czc_engine* e = new czc_engine();
  e->cfg = *cfg;
  e->dev = device_id;
  // precision 0: CLIP towers on bf16 MFMA; BERT on split-fp16 MFMA (hi+lo planes, three fp16 passes,
  // ~22 mantissa bits: the tau=0.1 softmax amplifies logit error tenfold, and BERT is 1.4% of the
  // FLOPs); 1: everything on f32 MFMA; 2: everything bf16 (experiments); 3: every tower on split-fp16 MFMA
  // 4: CLIP towers on single-pass fp16 MFMA (the bf16 kernels on IEEE fp16 operands), BERT on split-fp16
  // 5: screen-then-refine: CLIP-text screening pass on single-pass fp16, refine pass / vision tower / BERT on split-fp16
  e->refine = cfg->precision == CZC_PREC_REFINE;
  e->pc = cfg->precision == CZC_PREC_F32 ? PREC_F32
          : (cfg->precision == CZC_PREC_SPLIT ? PREC_F16X3
             : ((cfg->precision == CZC_PREC_FP16 || e->refine) ? PREC_F16 : PREC_BF16));
  e->pb = cfg->precision == CZC_PREC_ALL_BF16 ? PREC_BF16
                                              : (cfg->precision == CZC_PREC_F32 ? PREC_F32 : PREC_F16X3);
  e->pv = e->refine ? (int)PREC_F16X3 : e->pc;
  e->esz = prec_bytes(e->pc);
  e->eb = prec_bytes(e->pb);
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreate(&e->st) != hipSuccess ||
      hipHostMalloc((void**)&e->h_totals, 256) != hipSuccess) {
    snprintf(czc::g_err, sizeof(czc::g_err), "czc_create: stream/host allocation failed");
    delete e;
    return CZC_ERR_HIP;
  }
  memset(&e->bd, 0, sizeof(e->bd));
  *out = e;
  return CZC_OK;
}

int czc_destroy(czc_engine* e) {
  if (!e) return CZC_OK;
  (void)hipSetDevice(e->dev);
  (void)hipStreamSynchronize(e->st);
  if (e->shares_weights) { e->w.clear(); e->bert.clear(); e->ctext.clear(); e->cvis.clear(); e->ctext_x.clear();
                           e->mlm_dense_w = e->decoder_w = e->tproj_w = e->vproj_w = e->patch_w = e->tproj_wx = nullptr; }
  for (auto& kv : e->w) if (kv.second.p) (void)hipFree(kv.second.p);
  free_layer_set(e->bert); free_layer_set(e->ctext); free_layer_set(e->cvis); free_layer_set(e->ctext_x);
  (void)hipFree(e->mlm_dense_w); (void)hipFree(e->decoder_w); (void)hipFree(e->tproj_w); (void)hipFree(e->vproj_w);
  (void)hipFree(e->patch_w); (void)hipFree(e->tproj_wx);
  for (auto& kv : e->ws) if (kv.second.p) (void)hipFree(kv.second.p);
  for (void* p : e->bridge_allocs) (void)hipFree(p);
  (void)hipFree(e->d_mask); (void)hipFree(e->d_lex); (void)hipFree(e->d_lex_pos); (void)hipFree(e->d_lex_cls); (void)hipFree(e->d_img_n); (void)hipFree(e->d_staged);
  (void)hipFree(e->d_pos_tags); (void)hipFree(e->d_pos_masks);
  (void)hipFree(e->d_index);
  for (auto& kv : e->pk) for (hipEvent_t ev : kv.second.ev) (void)hipEventDestroy(ev);
  if (e->prof_ref) (void)hipEventDestroy(e->prof_ref);
  if (e->h_totals) (void)hipHostFree(e->h_totals);
  if (e->h_ctl_ids) (void)hipHostFree(e->h_ctl_ids);
  if (e->h_memo_list) (void)hipHostFree(e->h_memo_list);
  (void)hipStreamDestroy(e->st);
  delete e;
  return CZC_OK;
}

// A second engine on the same GPU over the SAME resident weights: its own stream, workspace, image embeddings,
// token mask / bridge / lexicon tables, options and profile.  Two (or three) of them driven from separate host
// threads polish disjoint image sub-batches concurrently: one sub-batch's small BERT / top-K / LayerNorm / attention
// launches and the tail rounds of its persistent GEMMs fill what the other's big launches leave idle.
int czc_replicate(czc_engine* p, czc_engine** out) {
  if (!p || !out) return CZC_ERR_ARG;
  if (!p->finalized) return fail(p, CZC_ERR_STATE, "czc_replicate: czc_finalize_weights first%s");
  czc_engine* e = new czc_engine();
  e->cfg = p->cfg; e->dev = p->dev; e->finalized = true; e->shares_weights = true;
  e->esz = p->esz; e->pb = p->pb; e->pc = p->pc; e->pv = p->pv; e->eb = p->eb;
  e->refine = p->refine; e->refine_theta_x = p->refine_theta_x; e->refine_samples = p->refine_samples; e->refine_samples_step = p->refine_samples_step;
  e->refine_guard_dev = p->refine_guard_dev; e->refine_gate_delta = p->refine_gate_delta; e->refine_theta_gen = p->refine_theta_gen;
  e->refine_rows16 = p->refine_rows16; e->refine_rows16_factor = p->refine_rows16_factor;
  e->memo = p->memo; e->memo_rows = p->memo_rows; e->fluency_chunk = p->fluency_chunk; e->regions_chunk = p->regions_chunk;
  e->w = p->w; e->bert = p->bert; e->ctext = p->ctext; e->cvis = p->cvis; e->ctext_x = p->ctext_x;
  e->mlm_dense_w = p->mlm_dense_w; e->decoder_w = p->decoder_w; e->tproj_w = p->tproj_w; e->vproj_w = p->vproj_w;
  e->patch_w = p->patch_w; e->tproj_wx = p->tproj_wx;
  e->logit_scale_exp = p->logit_scale_exp;
  e->share_prefix = p->share_prefix; e->dedup = p->dedup; e->pack_branches = p->pack_branches; e->pool_last_layer = p->pool_last_layer; e->pool_last_qkv = p->pool_last_qkv; e->share_layer0 = p->share_layer0;
  e->fuse_ln = p->fuse_ln; e->bert_prune = p->bert_prune; e->bert_fuse_splitk_ln = p->bert_fuse_splitk_ln; e->resid16 = p->resid16; e->fold_ln = p->fold_ln;
  memset(&e->bd, 0, sizeof(e->bd));
  if (hipSetDevice(e->dev) != hipSuccess || hipStreamCreate(&e->st) != hipSuccess ||
      hipHostMalloc((void**)&e->h_totals, 256) != hipSuccess) {
    e->w.clear();
    delete e;
    return fail(p, CZC_ERR_HIP, "czc_replicate: stream/host allocation failed%s");
  }
  *out = e;
  return CZC_OK;
}

int czc_load_tensor(czc_engine* e, const char* name, int dtype, int ndim, const int64_t* shape, const void* src) {
  if (e && e->shares_weights) return fail(e, CZC_ERR_STATE, "czc_load_tensor: a replica shares its parent's weights%s");
  if (!e || !name || !src || ndim < 0 || ndim > 8) return CZC_ERR_ARG;
  if (dtype != 0) return fail(e, CZC_ERR_ARG, "czc_load_tensor(%s): only fp32 (dtype 0) is accepted", name);
  E_HIP(hipSetDevice(e->dev));
  Tensor t;
  t.numel = 1;
  for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); t.numel *= (size_t)shape[i]; }
  auto it = e->w.find(name);
  if (it != e->w.end() && it->second.p) { (void)hipFree(it->second.p); }
  E_HIP(hipMalloc((void**)&t.p, t.numel * 4 + 16));
  E_HIP(hipMemcpy(t.p, src, t.numel * 4, hipMemcpyDefault));
  e->w[name] = t;
  e->finalized = false;
  return CZC_OK;
}

int czc_finalize_weights(czc_engine* e) {
  if (!e) return CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  const czc_config& c = e->cfg;
  const bool has_bert = c.bert_layers > 0 && c.bert_vocab > 0;
  if (e->shares_weights) return fail(e, CZC_ERR_STATE, "czc_finalize_weights: a replica shares its parent's weights%s");
  if (e->finalized) return CZC_OK;  // nothing loaded since the last call (czc_load_tensor clears the flag)
  E_HIP(hipStreamSynchronize(e->st));
  free_layer_set(e->bert); free_layer_set(e->ctext); free_layer_set(e->cvis); free_layer_set(e->ctext_x);
  for (void** p : {&e->mlm_dense_w, &e->decoder_w, &e->tproj_w, &e->vproj_w, &e->patch_w, &e->tproj_wx}) { (void)hipFree(*p); *p = nullptr; }
  if (has_bert) E_CHECK(build_layers(e, e->bert, c.bert_layers, c.bert_hidden, c.bert_inter, true, "bert.encoder.layer.", e->pb));
  E_CHECK(build_layers(e, e->ctext, c.clip_layers, c.clip_hidden, c.clip_inter, false, "text_model.encoder.layers.", e->pc));
  if (wants_folded_ln(e)) {  // folded-LayerNorm operands of the text tower (used where resid16 + fold_ln apply)
    const int H = c.clip_hidden, I = c.clip_inter;
    for (int n = 0; n < c.clip_layers; ++n) {
      LayerW& l = e->ctext[n];
      const std::string p = "text_model.encoder.layers." + std::to_string(n);
      float *qw, *kw, *vw, *f1w;
      E_CHECK(need(e, p + ".self_attn.q_proj.weight", (size_t)H * H, &qw));
      E_CHECK(need(e, p + ".self_attn.k_proj.weight", (size_t)H * H, &kw));
      E_CHECK(need(e, p + ".self_attn.v_proj.weight", (size_t)H * H, &vw));
      E_CHECK(need(e, p + ".mlp.fc1.weight", (size_t)I * H, &f1w));
      // (each pointer lands in the LayerW the moment it exists: czc_destroy / the next czc_finalize_weights frees whatever an
      // early return leaves behind)
      E_HIP(hipMalloc(&l.qkv_wf, (size_t)3 * H * H * 2));
      E_HIP(hipMalloc((void**)&l.qkv_bf, (size_t)3 * H * 4));
      E_HIP(hipMalloc(&l.fc1_wf, (size_t)I * H * 2));
      E_HIP(hipMalloc((void**)&l.fc1_bf, (size_t)I * 4));
      const float* srcw[3] = {qw, kw, vw};
      for (int t = 0; t < 3; ++t)
        E_CHECK(launch_fold_ln(srcw[t], l.ln1_g, l.ln1_b, l.qkv_b + t * H, H, H, (char*)l.qkv_wf + (size_t)t * H * H * 2, nullptr,
                               l.qkv_bf + t * H, e->st));
      E_CHECK(launch_fold_ln(f1w, l.ln2_g, l.ln2_b, l.fc1_b, I, H, l.fc1_wf, nullptr, l.fc1_bf, e->st));
    }
  }
  if (e->refine)
    E_CHECK(build_layers(e, e->ctext_x, c.clip_layers, c.clip_hidden, c.clip_inter, false, "text_model.encoder.layers.", PREC_F16X3));
  E_CHECK(build_layers(e, e->cvis, c.vis_layers, c.vis_hidden, c.vis_inter, false, "vision_model.encoder.layers.", e->pv));
  float* t;
  if (has_bert) {
    E_CHECK(need(e, "cls.predictions.transform.dense.weight", (size_t)c.bert_hidden * c.bert_hidden, &t));
    E_CHECK(to_act(e, e->pb, t, (size_t)c.bert_hidden * c.bert_hidden, &e->mlm_dense_w));
    // decoder weight tied to the word embeddings (HF:bert/modeling_bert.py:910-913)
    E_CHECK(need(e, "bert.embeddings.word_embeddings.weight", (size_t)c.bert_vocab * c.bert_hidden, &t));
    E_CHECK(to_act(e, e->pb, t, (size_t)c.bert_vocab * c.bert_hidden, &e->decoder_w));
    if (!find(e, "cls.predictions.bias") && find(e, "cls.predictions.decoder.bias")) {
      e->w["cls.predictions.bias"] = e->w["cls.predictions.decoder.bias"];
      e->w.erase("cls.predictions.decoder.bias");
    }
  }
  E_CHECK(need(e, "text_projection.weight", (size_t)c.clip_proj * c.clip_hidden, &t));
  E_CHECK(to_act(e, e->pc, t, (size_t)c.clip_proj * c.clip_hidden, &e->tproj_w));
  if (e->refine) E_CHECK(to_act(e, PREC_F16X3, t, (size_t)c.clip_proj * c.clip_hidden, &e->tproj_wx));
  E_CHECK(need(e, "visual_projection.weight", (size_t)c.clip_proj * c.vis_hidden, &t));
  E_CHECK(to_act(e, e->pv, t, (size_t)c.clip_proj * c.vis_hidden, &e->vproj_w));
  const size_t pk = (size_t)3 * c.vis_patch * c.vis_patch;
  E_CHECK(need(e, "vision_model.embeddings.patch_embedding.weight", (size_t)c.vis_hidden * pk, &t));
  E_CHECK(to_act(e, e->pv, t, (size_t)c.vis_hidden * pk, &e->patch_w));
  const Tensor* ls = find(e, "logit_scale");
  if (!ls) return fail(e, CZC_ERR_STATE, "missing tensor %s", "logit_scale");
  float lsv = 0.f;
  E_HIP(hipStreamSynchronize(e->st));
  E_HIP(hipMemcpy(&lsv, ls->p, 4, hipMemcpyDeviceToHost));
  e->logit_scale_exp = expf(lsv);
  // GEMM-operand masters are no longer needed (LN/bias/embedding tables stay fp32)
  std::vector<std::string> drop;
  for (auto& kv : e->w) {
    const std::string& n = kv.first;
    const bool is_w = n.size() > 7 && n.compare(n.size() - 7, 7, ".weight") == 0;
    const bool keep = n.find("LayerNorm") != std::string::npos || n.find("layer_norm") != std::string::npos ||
                      n.find("layrnorm") != std::string::npos || n.find("layernorm") != std::string::npos ||
                      n.find("embedding") != std::string::npos;
    if (is_w && !keep && kv.second.shape.size() == 2) drop.push_back(n);
  }
  for (auto& n : drop) { (void)hipFree(e->w[n].p); e->w.erase(n); }
  e->finalized = true;
  return CZC_OK;
}

int czc_set_token_mask(czc_engine* e, const float* mask, int vocab) {
  if (!e || !mask || vocab != e->cfg.bert_vocab) return e ? fail(e, CZC_ERR_ARG, "token mask size != bert_vocab%s") : CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  if (!e->d_mask) { E_HIP(hipMalloc((void**)&e->d_mask, (size_t)vocab * 4)); }
  E_HIP(hipMemcpy(e->d_mask, mask, (size_t)vocab * 4, hipMemcpyDefault));
  e->mask_vocab = vocab;
  return CZC_OK;
}

int czc_set_lexicon(czc_engine* e, const float* lex, int vocab) {
  if (!e || !lex || vocab != e->cfg.bert_vocab) return e ? fail(e, CZC_ERR_ARG, "lexicon size != bert_vocab%s") : CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  if (!e->d_lex) { E_HIP(hipMalloc((void**)&e->d_lex, (size_t)vocab * 4)); }
  E_HIP(hipMemcpy(e->d_lex, lex, (size_t)vocab * 4, hipMemcpyDefault));
  return CZC_OK;
}

int czc_set_lexicon_pos(czc_engine* e, const float* table, const uint8_t* class_of_token, int vocab) {
  if (!e) return CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  if (!table) {  // back to the per-token lexicon of czc_set_lexicon
    (void)hipFree(e->d_lex_pos); (void)hipFree(e->d_lex_cls);
    e->d_lex_pos = nullptr; e->d_lex_cls = nullptr;
    return CZC_OK;
  }
  if (!class_of_token || vocab != e->cfg.bert_vocab) return fail(e, CZC_ERR_ARG, "lexicon table size != bert_vocab%s");
  std::vector<uint8_t> cls(class_of_token, class_of_token + vocab);
  for (uint8_t c : cls) if (c > 4) return fail(e, CZC_ERR_ARG, "coarse POS class must be 0..4 ('' n v a r)%s");
  if (!e->d_lex_pos) E_HIP(hipMalloc((void**)&e->d_lex_pos, (size_t)vocab * 5 * 4));
  if (!e->d_lex_cls) E_HIP(hipMalloc((void**)&e->d_lex_cls, (size_t)vocab));
  E_HIP(hipMemcpy(e->d_lex_pos, table, (size_t)vocab * 5 * 4, hipMemcpyDefault));
  E_HIP(hipMemcpy(e->d_lex_cls, cls.data(), (size_t)vocab, hipMemcpyHostToDevice));
  return CZC_OK;
}

int czc_set_pos(czc_engine* e, const uint8_t* tag_of_token, int vocab, const uint16_t* template_masks, int n_template) {
  if (!e || !tag_of_token || !template_masks) return CZC_ERR_ARG;
  if (vocab != e->cfg.bert_vocab || n_template <= 0 || n_template > 32) return fail(e, CZC_ERR_ARG, "bad POS tables%s");
  E_HIP(hipSetDevice(e->dev));
  if (!e->d_pos_tags) E_HIP(hipMalloc((void**)&e->d_pos_tags, (size_t)vocab));
  if (!e->d_pos_masks) E_HIP(hipMalloc((void**)&e->d_pos_masks, 64));
  E_HIP(hipMemcpy(e->d_pos_tags, tag_of_token, (size_t)vocab, hipMemcpyDefault));
  E_HIP(hipMemcpy(e->d_pos_masks, template_masks, (size_t)n_template * 2, hipMemcpyDefault));
  e->pos_n = n_template;
  return CZC_OK;
}

static int upload(czc_engine* e, const void* src, size_t bytes, void** out) {
  void* p = nullptr;
  E_HIP(hipMalloc(&p, bytes + 16));
  E_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
  e->bridge_allocs.push_back(p);
  *out = p;
  return 0;
}

static int build_bridge(czc_engine* e, const czc_bridge_tables* t, BridgeDev* bd) {
  if (t->bert_vocab <= 0 || t->n_merges < 0) return fail(e, CZC_ERR_ARG, "bad bridge tables%s");
  const size_t nbytes = t->piece_off[t->bert_vocab];
  void* p;
  bd->bert_vocab = t->bert_vocab;
  E_CHECK(upload(e, t->piece_off, (size_t)(t->bert_vocab + 1) * 4, &p)); bd->piece_off = (const uint32_t*)p;
  E_CHECK(upload(e, t->piece_bytes, nbytes ? nbytes : 1, &p)); bd->piece_bytes = (const uint8_t*)p;
  E_CHECK(upload(e, t->piece_class, nbytes ? nbytes : 1, &p)); bd->piece_class = (const uint8_t*)p;
  E_CHECK(upload(e, t->piece_flags, (size_t)t->bert_vocab, &p)); bd->piece_flags = (const uint8_t*)p;
  E_CHECK(upload(e, t->byte_sym, 256 * 4, &p)); bd->byte_sym = (const int*)p;
  E_CHECK(upload(e, t->byte_sym_eow, 256 * 4, &p)); bd->byte_sym_eow = (const int*)p;
  size_t cap = 1024;
  while (cap < (size_t)t->n_merges * 2 + 2) cap <<= 1;
  std::vector<unsigned long long> keys(cap, ~0ull), vals(cap, 0ull);
  for (int r = 0; r < t->n_merges; ++r) {
    const unsigned long long key = ((unsigned long long)(unsigned)t->merge_left[r] << 32) | (unsigned)t->merge_right[r];
    unsigned h = bridge_hash(key) & (unsigned)(cap - 1);
    bool dup = false;
    while (keys[h] != ~0ull) {
      if (keys[h] == key) { dup = true; break; }  // first (lowest) rank wins
      h = (h + 1) & (unsigned)(cap - 1);
    }
    if (dup) continue;
    keys[h] = key;
    vals[h] = ((unsigned long long)(unsigned)r << 32) | (unsigned)t->merge_out[r];
  }
  E_CHECK(upload(e, keys.data(), cap * 8, &p)); bd->hkeys = (const unsigned long long*)p;
  E_CHECK(upload(e, vals.data(), cap * 8, &p)); bd->hvals = (const unsigned long long*)p;
  bd->hmask = (unsigned)(cap - 1);
  bd->bos_id = t->bos_id;
  bd->eos_id = t->eos_id;
  // ids of every all-letter token standing alone as a word, tabulated once by the same BPE code (bridge.hip)
  bd->tok_bpe = nullptr; bd->tok_bpe_len = nullptr;
  int* tok_ids = nullptr; uint8_t* tok_len = nullptr;
  E_HIP(hipMalloc((void**)&tok_ids, (size_t)t->bert_vocab * BR_TOKMAX * 4 + 16));
  e->bridge_allocs.push_back(tok_ids);
  E_HIP(hipMalloc((void**)&tok_len, (size_t)t->bert_vocab + 16));
  e->bridge_allocs.push_back(tok_len);
  E_CHECK(launch_bridge_precompute(*bd, tok_ids, tok_len, e->st));
  E_HIP(hipStreamSynchronize(e->st));
  bd->tok_bpe = tok_ids; bd->tok_bpe_len = tok_len;
  return 0;
}

int czc_set_bridge(czc_engine* e, const czc_bridge_tables* t) {
  if (!e || !t) return CZC_ERR_ARG;
  if (t->bert_vocab != e->cfg.bert_vocab) return fail(e, CZC_ERR_ARG, "bridge bert_vocab != config%s");
  E_HIP(hipSetDevice(e->dev));
  for (void* p : e->bridge_allocs) (void)hipFree(p);
  e->bridge_allocs.clear();
  E_CHECK(build_bridge(e, t, &e->bd));
  e->has_bridge = true;
  return CZC_OK;
}

int czc_set_image_embeds(czc_engine* e, const float* embeds, int B) {
  if (!e || !embeds || B <= 0) return CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  const int D = e->cfg.clip_proj;
  float* raw;
  E_CHECK(ensure(e, "img_raw", (size_t)B * D * 4, (void**)&raw));
  E_HIP(hipMemcpyAsync(raw, embeds, (size_t)B * D * 4, hipMemcpyDefault, e->st));
  if (e->img_B < B) { if (e->d_img_n) (void)hipFree(e->d_img_n); e->d_img_n = nullptr; E_HIP(hipMalloc((void**)&e->d_img_n, (size_t)B * D * 4)); }
  E_CHECK(launch_l2_normalize(raw, B, D, e->d_img_n, e->st));
  e->img_B = B;
  E_HIP(hipStreamSynchronize(e->st));
  return CZC_OK;
}

int czc_encode_images(czc_engine* e, const float* pixels, int B, float* out_embeds) {
  if (!e || !pixels || B <= 0) return CZC_ERR_ARG;
  if (!e->finalized) return fail(e, CZC_ERR_STATE, "weights not finalized%s");
  E_HIP(hipSetDevice(e->dev));
  const czc_config& c = e->cfg;
  const int P = e->pv, S = c.vis_image, p = c.vis_patch, G = S / p, NP = G * G, H = c.vis_hidden;
  const size_t vsz = prec_bytes(P);
  const int Kc = 3 * p * p, T = NP + 1, M = B * T;
  float *pix, *pe, *x, *emb; void *patches, *ca; int* idx;
  E_CHECK(ensure(e, "v_pix", (size_t)B * 3 * S * S * 4, (void**)&pix));
  E_CHECK(ensure(e, "v_patches", (size_t)B * NP * Kc * vsz, &patches));
  E_CHECK(ensure(e, "v_pe", (size_t)B * NP * H * 4, (void**)&pe));
  E_CHECK(ensure(e, "v_x", (size_t)M * H * 4, (void**)&x));
  E_CHECK(ensure(e, "v_idx", (size_t)B * 4, (void**)&idx));
  E_CHECK(ensure(e, "v_ca", (size_t)B * H * vsz, &ca));
  E_CHECK(ensure(e, "img_raw", (size_t)B * c.clip_proj * 4, (void**)&emb));
  E_HIP(hipMemcpyAsync(pix, pixels, (size_t)B * 3 * S * S * 4, hipMemcpyDefault, e->st));
  float *cls, *pos, *g0, *b0, *g1, *b1;
  E_CHECK(need(e, "vision_model.embeddings.class_embedding", H, &cls));
  E_CHECK(need(e, "vision_model.embeddings.position_embedding.weight", (size_t)T * H, &pos));
  E_CHECK(need(e, "vision_model.pre_layrnorm.weight", H, &g0));
  E_CHECK(need(e, "vision_model.pre_layrnorm.bias", H, &b0));
  E_CHECK(need(e, "vision_model.post_layernorm.weight", H, &g1));
  E_CHECK(need(e, "vision_model.post_layernorm.bias", H, &b1));
  { ProfScope ps(e, "rowops", 0); E_CHECK(launch_im2col(P, pix, B, S, p, patches, e->st)); }
  E_CHECK(gemm(e, P, "gemm_vision", patches, Kc, e->patch_w, Kc, nullptr, nullptr, 0, nullptr, pe, H, B * NP, H, Kc, ACT_NONE));
  { ProfScope ps(e, "rowops", 0);
    E_CHECK(launch_vision_assemble(pe, B, NP, H, cls, pos, x, e->st));
    E_CHECK(launch_layernorm(P, x, nullptr, g0, b0, c.clip_eps, M, H, nullptr, x, e->st)); }
  SegTable vtab{nullptr, nullptr, nullptr, nullptr, B, T};
  E_CHECK(clip_stack(e, StackDesc{P, &e->cvis, "gemm_vision", M, H, c.vis_inter, c.vis_heads, c.clip_eps, vtab, T, 0}, x));
  { ProfScope ps(e, "rowops", 0);
    E_CHECK(launch_make_row_index(idx, B, T, 0, e->st));
    E_CHECK(launch_layernorm(P, x, idx, g1, b1, c.clip_eps, B, H, ca, nullptr, e->st)); }
  E_CHECK(gemm(e, P, "gemm_vision", ca, H, e->vproj_w, H, nullptr, nullptr, 0, nullptr, emb, c.clip_proj, B, c.clip_proj, H, ACT_NONE));
  if (e->img_B < B) { if (e->d_img_n) (void)hipFree(e->d_img_n); e->d_img_n = nullptr; E_HIP(hipMalloc((void**)&e->d_img_n, (size_t)B * c.clip_proj * 4)); }
  E_CHECK(launch_l2_normalize(emb, B, c.clip_proj, e->d_img_n, e->st));
  e->img_B = B;
  if (out_embeds) E_HIP(hipMemcpyAsync(out_embeds, emb, (size_t)B * c.clip_proj * 4, hipMemcpyDefault, e->st));
  E_HIP(hipStreamSynchronize(e->st));
  return CZC_OK;
}

int czc_preprocess_u8(czc_engine* e, const uint8_t* rgb, int height, int width, const float* mean, const float* stdv,
                      int slot, float* pixels_out) {
  if (!e || !rgb || !mean || !stdv || slot < 0) return CZC_ERR_ARG;
  if (height <= 0 || width <= 0 || (long)height * width > (1L << 28)) return fail(e, CZC_ERR_ARG, "preprocess: bad image size%s");
  E_HIP(hipSetDevice(e->dev));
  const int S = e->cfg.vis_image;
  const size_t img = (size_t)3 * S * S;
  // staged batch grows by doubling and keeps its contents
  if (slot >= e->staged_cap) {
    int cap = e->staged_cap ? e->staged_cap : 8;
    while (cap <= slot) cap *= 2;
    float* nb = nullptr;
    E_HIP(hipMalloc((void**)&nb, (size_t)cap * img * 4));
    if (e->d_staged) {
      E_HIP(hipMemcpyAsync(nb, e->d_staged, (size_t)e->staged_cap * img * 4, hipMemcpyDeviceToDevice, e->st));
      E_HIP(hipStreamSynchronize(e->st));
      E_HIP(hipFree(e->d_staged));
    }
    e->d_staged = nb;
    e->staged_cap = cap;
  }
  unsigned char *d_rgb, *scratch;
  E_CHECK(ensure(e, "pp_rgb", (size_t)height * width * 3, (void**)&d_rgb));
  E_CHECK(ensure(e, "pp_scratch", imageproc_scratch_bytes(height, width, S), (void**)&scratch));
  E_HIP(hipMemcpyAsync(d_rgb, rgb, (size_t)height * width * 3, hipMemcpyDefault, e->st));
  float* dst = e->d_staged + (size_t)slot * img;
  {
    ProfScope ps(e, "rowops", 0);
    if (launch_clip_preprocess(d_rgb, height, width, S, mean, stdv, scratch, dst, e->st)) return fail(e, CZC_ERR_HIP, "%s", g_err);
  }
  if (pixels_out) E_HIP(hipMemcpyAsync(pixels_out, dst, img * 4, hipMemcpyDefault, e->st));
  E_HIP(hipStreamSynchronize(e->st));
  if (slot + 1 > e->staged_n) e->staged_n = slot + 1;
  return CZC_OK;
}

// N boxes of one image into staged slots slot0 .. slot0 + n - 1: slot slot0 + i = czc_preprocess_u8 of the contiguous copy of
// rgb[y0:y1, x0:x1], bit for bit.  One upload of the image; per chunk of "regions_chunk" boxes one upload of descriptors and
// window tables, two launches and one synchronisation (the chunk's host staging must have left before it is rebuilt).
int czc_preprocess_regions_u8(czc_engine* e, const uint8_t* rgb, int height, int width, const int32_t* boxes, int n, const float* mean,
                              const float* stdv, int slot0, float* pixels_out) {
  if (!e) return CZC_ERR_ARG;
  if (!rgb || !boxes || !mean || !stdv) return fail(e, CZC_ERR_ARG, "preprocess_regions: null argument%s");
  if (n < 1 || n > CZC_MAX_REGIONS) return fail(e, CZC_ERR_ARG, "preprocess_regions: the number of regions is outside [1, 1024]%s");
  if (slot0 < 0) return fail(e, CZC_ERR_ARG, "preprocess_regions: slot0 is negative%s");
  if (slot0 > (1 << 20)) return fail(e, CZC_ERR_ARG, "preprocess_regions: slot0 above 2^20%s");  // (slot0 + n stays an int)
  if (height <= 0 || width <= 0 || (long)height * width > (1L << 28)) return fail(e, CZC_ERR_ARG, "preprocess_regions: bad image size%s");
  const int S = e->cfg.vis_image;
  for (int i = 0; i < n; ++i) {
    const int x0 = boxes[4 * i], y0 = boxes[4 * i + 1], x1 = boxes[4 * i + 2], y1 = boxes[4 * i + 3];
    if (x0 < 0 || y0 < 0 || x1 > width || y1 > height || x0 >= x1 || y0 >= y1) {
      snprintf(e->err, sizeof(e->err), "preprocess_regions: box %d = (%d, %d, %d, %d) is empty or leaves the %dx%d image", i, x0, y0, x1,
               y1, width, height);
      return CZC_ERR_ARG;
    }
    const int bw = x1 - x0, bh = y1 - y0;
    const double longest = bw <= bh ? (double)S * bh / bw : (double)S * bw / bh;
    if (longest > (double)(1 << 24)) {
      snprintf(e->err, sizeof(e->err), "preprocess_regions: box %d = (%d, %d, %d, %d) resizes to a long side above 2^24", i, x0, y0, x1, y1);
      return CZC_ERR_ARG;
    }
  }
  E_HIP(hipSetDevice(e->dev));
  const size_t img = (size_t)3 * S * S;
  // the plans first: a chunk that cannot be laid out refuses the call before the staged batch is touched
  const int chunk = e->regions_chunk, n_chunk = (n + chunk - 1) / chunk;
  std::vector<RegionsPlan> plans((size_t)n_chunk);
  size_t scratch_bytes = 0;
  for (int c = 0; c < n_chunk; ++c) {
    const int lo = c * chunk, cnt = std::min(chunk, n - lo);
    if (plan_clip_regions(S, boxes + 4 * (size_t)lo, cnt, plans[c])) return fail(e, CZC_ERR_ARG, "%s", g_err);
    scratch_bytes = std::max(scratch_bytes, plans[c].scratch_bytes);
  }
  // staged batch grows by doubling and keeps its contents
  if (slot0 + n > e->staged_cap) {
    int cap = e->staged_cap ? e->staged_cap : 8;
    while (cap < slot0 + n) cap *= 2;
    float* nb = nullptr;
    E_HIP(hipMalloc((void**)&nb, (size_t)cap * img * 4));
    if (e->d_staged) {
      E_HIP(hipMemcpyAsync(nb, e->d_staged, (size_t)e->staged_cap * img * 4, hipMemcpyDeviceToDevice, e->st));
      E_HIP(hipStreamSynchronize(e->st));
      E_HIP(hipFree(e->d_staged));
    }
    e->d_staged = nb;
    e->staged_cap = cap;
  }
  unsigned char *d_rgb, *scratch;
  E_CHECK(ensure(e, "pp_rgb", (size_t)height * width * 3, (void**)&d_rgb));
  E_CHECK(ensure(e, "pp_scratch", scratch_bytes, (void**)&scratch));
  E_HIP(hipMemcpyAsync(d_rgb, rgb, (size_t)height * width * 3, hipMemcpyDefault, e->st));
  float* dst = e->d_staged + (size_t)slot0 * img;
  for (int c = 0; c < n_chunk; ++c) {
    {
      ProfScope ps(e, "rowops", 0);
      if (launch_clip_regions(d_rgb, width, S, plans[c], mean, stdv, scratch, dst + (size_t)c * chunk * img, e->st))
        return fail(e, CZC_ERR_HIP, "%s", g_err);
    }
    // the next chunk overwrites the scratch in stream order; the host only waits where it frees a chunk's staging early
    if (c + 1 < n_chunk) {
      E_HIP(hipStreamSynchronize(e->st));
      std::vector<unsigned char>().swap(plans[c].host);
    }
  }
  if (pixels_out) E_HIP(hipMemcpyAsync(pixels_out, dst, (size_t)n * img * 4, hipMemcpyDefault, e->st));
  E_HIP(hipStreamSynchronize(e->st));
  if (slot0 + n > e->staged_n) e->staged_n = slot0 + n;
  return CZC_OK;
}

int czc_encode_staged(czc_engine* e, int B, float* out_embeds) {
  if (!e || B <= 0) return CZC_ERR_ARG;
  if (B > e->staged_n) return fail(e, CZC_ERR_STATE, "encode_staged: fewer staged images than requested%s");
  return czc_encode_images(e, e->d_staged, B, out_embeds);
}

// host CLIP id rows of B x K sequences through the engine's own plan and text tower -> features [B * K, proj] on the host
static int text_features(czc_engine* e, const int32_t* clip_ids, const int32_t* clip_len, int B, int K, int share, bool exact, float* out,
                         TowerPlan* tp = nullptr) {
  if (!e->finalized) return fail(e, CZC_ERR_STATE, "weights not finalized%s");
  E_HIP(hipSetDevice(e->dev));
  e->err[0] = 0;
  const int n = B * K;
  int *cids, *clen, *totals;
  E_CHECK(ensure(e, "s_cids", (size_t)n * CZC_CLIP_MAX_LEN * 4, (void**)&cids));
  E_CHECK(ensure(e, "s_clen", (size_t)n * 4, (void**)&clen));
  E_CHECK(ensure(e, "s_tot", PLAN_TOTALS, (void**)&totals));
  E_HIP(hipMemcpyAsync(cids, clip_ids, (size_t)n * CZC_CLIP_MAX_LEN * 4, hipMemcpyDefault, e->st));
  E_HIP(hipMemcpyAsync(clen, clip_len, (size_t)n * 4, hipMemcpyDefault, e->st));
  E_HIP(hipMemsetAsync(totals, 0, PLAN_TOTALS, e->st));
  { int* flag; E_CHECK(ensure(e, "s_nonfinite", 32, (void**)&flag)); E_HIP(hipMemsetAsync(flag, 0, 32, e->st)); }
  float* feat;
  E_CHECK(clip_text_forward(e, cids, clen, B, K, share, totals, &feat, exact, tp));
  E_HIP(hipMemcpyAsync(out, feat, (size_t)n * e->cfg.clip_proj * 4, hipMemcpyDefault, e->st));
  E_HIP(hipStreamSynchronize(e->st));
  return CZC_OK;
}

int czc_encode_text(czc_engine* e, const int32_t* clip_ids, const int32_t* clip_len, int n, float* out_embeds) {
  if (!e || !clip_ids || !clip_len || n <= 0 || !out_embeds) return CZC_ERR_ARG;
  return text_features(e, clip_ids, clip_len, n, 1, 0, true, out_embeds);  // independent sequences: no sharing; exact tower
}

// clip/clip.py:86-98 `compute_image_text_similarity_via_embeddings` as a call of its own (the per-step path never needs it:
// czc_step / czc_generate fuse it into the score-combine kernel; this is the drop-in CLIP wrapper's public method): both sides
// L2-normalised, cos = t . i, logits = cos * exp(logit_scale) of the loaded checkpoint, softmax over the K texts of an image.
int czc_similarity(czc_engine* e, const float* image_embeds, const float* text_embeds, int B, int K, float* clip_score,
                   float* clip_ref) {
  if (!e || !image_embeds || !text_embeds || B <= 0 || K <= 0 || K > CZC_MAX_TOPK) return e ? fail(e, CZC_ERR_ARG, "similarity: bad B / K%s") : CZC_ERR_ARG;
  if (!e->finalized) return fail(e, CZC_ERR_STATE, "weights not finalized%s");
  E_HIP(hipSetDevice(e->dev));
  e->err[0] = 0;
  const int D = e->cfg.clip_proj;
  const size_t bk = (size_t)B * K;
  float *tf, *ie, *in_, *zero, *cs, *cr, *fin, *bc; int *cand, *best, *flag;
  E_CHECK(ensure(e, "sim_tf", bk * D * 4, (void**)&tf));
  E_CHECK(ensure(e, "sim_ie", (size_t)B * D * 4, (void**)&ie));
  E_CHECK(ensure(e, "sim_in", (size_t)B * D * 4, (void**)&in_));
  E_CHECK(ensure(e, "sim_zero", bk * 4, (void**)&zero));
  E_CHECK(ensure(e, "sim_cand", bk * 4, (void**)&cand));
  E_CHECK(ensure(e, "sim_cs", bk * 4, (void**)&cs));
  E_CHECK(ensure(e, "sim_cr", bk * 4, (void**)&cr));
  E_CHECK(ensure(e, "sim_fin", bk * 4, (void**)&fin));
  E_CHECK(ensure(e, "sim_best", (size_t)B * 4, (void**)&best));
  E_CHECK(ensure(e, "sim_bc", (size_t)B * 4, (void**)&bc));
  E_CHECK(ensure(e, "sim_flag", 32, (void**)&flag));
  E_HIP(hipMemcpyAsync(tf, text_embeds, bk * D * 4, hipMemcpyDefault, e->st));
  E_HIP(hipMemcpyAsync(ie, image_embeds, (size_t)B * D * 4, hipMemcpyDefault, e->st));
  E_HIP(hipMemsetAsync(zero, 0, bk * 4, e->st));
  E_HIP(hipMemsetAsync(cand, 0, bk * 4, e->st));
  E_HIP(hipMemsetAsync(flag, 0, 32, e->st));
  E_CHECK(launch_l2_normalize(ie, B, D, in_, e->st));
  CombineArgs a;
  a.text_feat = tf; a.img_n = in_; a.logit_scale_exp = e->logit_scale_exp; a.probs = zero; a.cand = cand;
  a.senti_raw = nullptr; a.repeats = nullptr; a.alpha = 0.f; a.beta = 1.f; a.gamma = 0.f; a.use_senti = 0;
  a.B = B; a.K = K; a.D = D; a.clip_score = cs; a.clip_ref = cr; a.final_score = fin; a.best = best; a.best_cos = bc;
  a.inp = nullptr; a.T = 0; a.gen_idx = 0; a.nonfinite = flag;
  E_CHECK(launch_combine(a, e->st));
  if (clip_score) E_HIP(hipMemcpyAsync(clip_score, cs, bk * 4, hipMemcpyDefault, e->st));
  if (clip_ref) E_HIP(hipMemcpyAsync(clip_ref, cr, bk * 4, hipMemcpyDefault, e->st));
  E_HIP(hipStreamSynchronize(e->st));
  return CZC_OK;
}

// ---- caption retrieval: the resident text index and its search (retrieve.hip) ---------------------------------------------------
namespace {
bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }  // plain host memory: not registered
  return a.type == hipMemoryTypeDevice;
}
}  // namespace

int czc_index_set(czc_engine* e, const float* embeds, int64_t n) {
  if (!e || n < 0) return CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  e->err[0] = 0;
  if (!embeds || n == 0) {
    E_HIP(hipStreamSynchronize(e->st));
    if (e->d_index) (void)hipFree(e->d_index);
    e->d_index = nullptr; e->index_n = 0;
    return CZC_OK;
  }
  const int D = e->cfg.clip_proj;
  if (D <= 0 || D % 32 || D > 1024) return fail(e, CZC_ERR_ARG, "czc_index_set: clip_proj must be a multiple of 32 and at most 1024%s");
  // ids are int32, and the scan's block indices run up to one stride (1024 work-groups x 4 blocks x 32 rows) past n
  if (n > (int64_t)INT32_MAX - (1 << 18)) return fail(e, CZC_ERR_ARG, "czc_index_set: too many rows for int32 ids%s");
  const size_t row_b = (size_t)D * 4;
  split_t* fresh = nullptr;
  int* flag = nullptr;
  E_CHECK(ensure(e, "ix_flag", 32, (void**)&flag));
  if (hipMalloc((void**)&fresh, (size_t)n * row_b) != hipSuccess) {
    (void)hipGetLastError();
    snprintf(e->err, sizeof(e->err), "czc_index_set: cannot allocate %zu bytes for %lld rows", (size_t)n * row_b, (long long)n);
    return CZC_ERR_HIP;
  }
  int rc = 0, bad = 0;
  auto run = [&]() -> int {
    E_HIP(hipMemsetAsync(flag, 0, 4, e->st));
    if (is_device_ptr(embeds)) {
      E_CHECK(launch_normalize_split(embeds, n, D, fresh, flag, 0, e->st));
    } else {
      // host rows pass through a staging buffer of at most 64 MiB; each row is still read once by the kernel
      const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)64 << 20) / (int64_t)row_b));
      float* stage;
      E_CHECK(ensure(e, "ix_stage", (size_t)chunk * row_b, (void**)&stage));
      for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        E_HIP(hipMemcpyAsync(stage, embeds + r0 * D, (size_t)m * row_b, hipMemcpyDefault, e->st));
        E_CHECK(launch_normalize_split(stage, m, D, (split_t*)((unsigned char*)fresh + (size_t)r0 * row_b), flag, 0, e->st));
        E_HIP(hipStreamSynchronize(e->st));  // the pageable source of the next copy must not overtake this kernel's read
      }
    }
    E_HIP(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, e->st));
    E_HIP(hipStreamSynchronize(e->st));
    return 0;
  };
  rc = run();
  if (!rc && bad) rc = fail(e, CZC_ERR_ARG, "czc_index_set: a row has norm 0 or is not finite; the previous index stays%s");
  if (rc) { (void)hipFree(fresh); return rc; }
  if (e->d_index) (void)hipFree(e->d_index);
  e->d_index = fresh; e->index_n = n;
  return CZC_OK;
}

int czc_index_size(czc_engine* e, int64_t* n) {
  if (!e || !n) return CZC_ERR_ARG;
  *n = e->d_index ? e->index_n : 0;
  return CZC_OK;
}

int czc_index_search(czc_engine* e, const float* image_embeds, int Q, int k, int32_t* out_ids, float* out_cos) {
  if (!e || !out_ids || !out_cos) return CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  e->err[0] = 0;
  if (k < 1 || k > CZC_INDEX_MAX_K || Q < 1) return fail(e, CZC_ERR_ARG, "czc_index_search: need Q >= 1 and 1 <= k <= CZC_INDEX_MAX_K%s");
  if (!e->d_index) return fail(e, CZC_ERR_STATE, "czc_index_search: no index (czc_index_set first)%s");
  const int D = e->cfg.clip_proj;
  const int n = (int)e->index_n;
  const float* src = image_embeds;
  if (!src) {
    auto it = e->ws.find("img_raw");
    if (e->img_B <= 0 || it == e->ws.end() || !it->second.p) return fail(e, CZC_ERR_STATE, "czc_index_search: no resident image embeddings%s");
    if (Q > e->img_B) return fail(e, CZC_ERR_ARG, "czc_index_search: Q exceeds the resident image embeddings%s");
    src = (const float*)it->second.p;
  } else if (!is_device_ptr(src)) {
    float* raw;
    E_CHECK(ensure(e, "ix_qraw", (size_t)Q * D * 4, (void**)&raw));
    E_HIP(hipMemcpyAsync(raw, src, (size_t)Q * D * 4, hipMemcpyDefault, e->st));
    src = raw;
  }
  const int G = index_scan_groups(n, D, k, e->index_groups);
  const size_t qk = (size_t)Q * k;
  split_t* qs; unsigned long long* part; int32_t* out;
  E_CHECK(ensure(e, "ix_qs", (size_t)Q * D * 4, (void**)&qs));
  E_CHECK(ensure(e, "ix_part", qk * G * 8, (void**)&part));
  E_CHECK(ensure(e, "ix_out", (2 * qk + Q) * 4, (void**)&out));  // ids [Q, k] | cosines [Q, k] | bad-query flags [Q]: one read
  E_CHECK(launch_normalize_split(src, Q, D, qs, out + 2 * qk, 1, e->st));
  E_CHECK(launch_index_search(e->d_index, n, D, qs, Q, k, G, part, out, (float*)(out + qk), e->st));
  std::vector<int32_t> host(2 * qk + Q);
  E_HIP(hipMemcpyAsync(host.data(), out, host.size() * 4, hipMemcpyDeviceToHost, e->st));
  E_HIP(hipStreamSynchronize(e->st));
  for (int q = 0; q < Q; ++q)
    if (host[2 * qk + q]) return fail(e, CZC_ERR_ARG, "czc_index_search: a query row has norm 0 or is not finite%s");
  memcpy(out_ids, host.data(), qk * 4);
  memcpy(out_cos, host.data() + qk, qk * 4);
  return CZC_OK;
}

int czc_step(czc_engine* e, int32_t* inp, int B, int T, int gen_idx, int n_mask, int dot_allowed, int top_k,
             const czc_hyper* hp, const czc_step_out* out) {
  if (!e || !inp || !hp || B <= 0) return CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  e->err[0] = 0;
  int* d_inp;
  { int* flag; E_CHECK(ensure(e, "s_nonfinite", 32, (void**)&flag)); E_HIP(hipMemsetAsync(flag, 0, 32, e->st)); }
  E_CHECK(ensure(e, "g_inp", (size_t)B * T * 4, (void**)&d_inp));
  E_HIP(hipMemcpyAsync(d_inp, inp, (size_t)B * T * 4, hipMemcpyDefault, e->st));
  StepArgs a{d_inp, B, T, gen_idx, n_mask, dot_allowed, top_k, *hp};
  // parity granularity: every one of the K fused scores is an output, all of them are refined -- no gate (need_cos is read on the
  // gated path only: its default)
  a.img = resident_images(e, B); a.mode = StepMode{false, false, true};
  E_CHECK(step_device(e, a));
  const size_t bk = (size_t)B * top_k;
  if (out) {
    E_CHECK(copy_out(e, out->probs, "s_probs", bk * 4));
    E_CHECK(copy_out(e, out->idxs, "s_idxs", bk * 4));
    E_CHECK(copy_out(e, out->cand_ids, "s_cand", bk * 4));
    E_CHECK(copy_out(e, out->clip_ids, "s_cids", bk * CZC_CLIP_MAX_LEN * 4));
    E_CHECK(copy_out(e, out->clip_len, "s_clen", bk * 4));
    E_CHECK(copy_out(e, out->clip_score, "s_cscore", bk * 4));
    E_CHECK(copy_out(e, out->clip_ref, "s_cref", bk * 4));
    E_CHECK(copy_out(e, out->senti_raw, "s_senti", bk * 4));
    E_CHECK(copy_out(e, out->repeats, "s_reps", bk * 4));
    E_CHECK(copy_out(e, out->final_score, "s_fin", bk * 4));
    E_CHECK(copy_out(e, out->best, "s_best", (size_t)B * 4));
    E_CHECK(copy_out(e, out->best_cos, "s_bcos", (size_t)B * 4));
    E_CHECK(copy_out(e, out->logits, "b_logits", (size_t)B * e->cfg.bert_vocab * 4));
  }
  E_HIP(hipMemcpyAsync(inp, d_inp, (size_t)B * T * 4, hipMemcpyDefault, e->st));
  return finish_steps(e);
}

// ---- czc_generate and the czc_generate_rows* family --------------------------------------------------------------------
// rows = false (czc_generate): positions [n_steps], one column for the whole batch at every step (the scalar kernels, the memo
// where the option is on).  rows = true: positions [n_steps, R], image_of_row [R] or null; the schedule (SchedLayout) is uploaded
// once and every step reads its slice.  from = true: init is [R, T], one start row per row, and a position may be CZC_POS_IDLE; a
// call with idle steps takes the compact-batch path of memo_rows_step (with the entries where option "memo_rows" is on, without
// them otherwise), a call without any runs as czc_generate_rows does.  len (rows that differ in length; null otherwise): row r
// polishes len[r] positions and holds seed_len + len[r] + 1 tokens, T is the stride of the rows and L the longest length; BERT,
// the MLM head's row index and the bridge then run on the packed rows (Ragged).

// The checks every generate call passes, on the call as the check_* functions left it; *any_idle: some row sits a step out
static int check_call(czc_engine* e, const RowsCall& c, bool* any_idle) {
  const int B = c.R, T = c.T, L = c.L, n_steps = c.n_steps;
  const int32_t *pos = c.positions, *len = c.len;
  if (!e || !c.init || !pos || !c.hp || B <= 0 || n_steps < 0 || c.snapshot_every <= 0) return CZC_ERR_ARG;
  if (c.seed_len + L > T) return fail(e, CZC_ERR_ARG, "generate: seed_len + L > T%s");
  E_HIP(hipSetDevice(e->dev));
  e->err[0] = 0;
  const size_t n_pos = c.n_pos();
  for (size_t i = 0; i < n_pos; ++i)
    if (pos[i] < (c.from ? CZC_POS_IDLE : 0) || pos[i] >= L)  // (len mode: checked per row by check_lengths)
      return fail(e, CZC_ERR_ARG, c.from ? "generate_rows_from: position outside {CZC_POS_IDLE} and [0, L)%s" : "generate: position out of range%s");
  *any_idle = false;
  if (c.from) {
    for (size_t i = 0; i < (size_t)B * T; ++i)
      if (c.init[i] < 0 || c.init[i] >= e->cfg.bert_vocab)
        return fail(e, CZC_ERR_ARG, "generate_rows_from: start row holds an id outside the BERT vocabulary%s");
    for (int s = 0; s < n_steps;) {  // a group: an n_mask >= 1 step plus the n_mask = 0 steps behind it
      int g = 1;
      while (s + g < n_steps && c.n_mask && c.n_mask[s + g] <= 0) ++g;
      for (int r = 0; r < B; ++r) {
        const bool idle = pos[(size_t)s * B + r] == CZC_POS_IDLE;
        *any_idle = *any_idle || idle;
        for (int j = 1; j < g; ++j)
          if ((pos[(size_t)(s + j) * B + r] == CZC_POS_IDLE) != idle)
            return fail(e, CZC_ERR_ARG, "generate_rows_from: a row must be idle for a whole step group (an n_mask >= 1 step and the n_mask = 0 steps behind it) or for none of it%s");
      }
      s += g;
    }
  }
  if (c.rows) {
    if (B > CZC_MAX_ROWS || c.seed_len < 0 || T > CZC_MAX_BERT_LEN) return fail(e, CZC_ERR_ARG, "generate_rows: R > CZC_MAX_ROWS, seed_len < 0 or T > CZC_MAX_BERT_LEN%s");
    if (!e->d_img_n || e->img_B <= 0) return fail(e, CZC_ERR_STATE, "image embeds not set%s");
    if (!c.image_of_row && e->img_B != B)
      return fail(e, CZC_ERR_ARG, "generate_rows: image_of_row = NULL needs R equal to the resident image batch%s");
    if (c.image_of_row)
      for (int r = 0; r < B; ++r)
        if (c.image_of_row[r] < 0 || c.image_of_row[r] >= e->img_B)
          return fail(e, CZC_ERR_ARG, "generate_rows: image_of_row outside the resident image batch%s");
    if (e->ctl_fn && c.hp->control && c.from) {  // the callback sees the rows that run, compacted: those must share one position
      for (int s = 0; s < n_steps; ++s) {
        int shared = CZC_POS_IDLE, first_r = 0;
        for (int r = 0; r < B; ++r) {
          const int p = pos[(size_t)s * B + r];
          if (p == CZC_POS_IDLE) continue;
          // (the length is compared only between rows at one position: a row at another position is refused just below)
          if (shared != CZC_POS_IDLE && p == shared && len && len[r] != len[first_r])
            return fail(e, CZC_ERR_ARG, "generate_rows_len: a control callback is told one T, so the rows of a step that are not idle must share one length as well "
                                        "as one position; use the control tables (czc_set_lexicon / czc_set_lexicon_pos / czc_set_pos)%s");
          if (shared == CZC_POS_IDLE) first_r = r;
          if (shared != CZC_POS_IDLE && p != shared)
            return fail(e, CZC_ERR_ARG, "generate_rows_from: a control callback carries one gen_idx, so the rows that are not idle must visit the same position at a step; "
                                        "use the control tables (czc_set_lexicon / czc_set_lexicon_pos / czc_set_pos)%s");
          shared = p;
        }
      }
    } else if (e->ctl_fn && c.hp->control)  // the callback is only called on controlled steps
      for (size_t i = 0; i < n_pos; ++i)
        if (pos[i] != pos[i - i % B])
          return fail(e, CZC_ERR_ARG, "generate_rows: a control callback carries one gen_idx, so every row must visit the same position at a step; "
                                      "use the control tables (czc_set_lexicon / czc_set_lexicon_pos / czc_set_pos) or one czc_generate call per order%s");
  }
  return 0;
}

// The schedule of a rows call on the host, with its layout (czc_generate has none: its one column travels as an argument)
static Sched build_schedule(const RowsCall& c, bool any_idle) {
  Sched sc;
  if (!c.rows) return sc;
  const int B = c.R, n_steps = c.n_steps;
  const int32_t* pos = c.positions;
  const size_t n_pos = c.n_pos();
  SchedLayout& at = sc.at;
  at.R = B; at.idle = any_idle; at.dot = n_pos; at.run = 2 * n_pos; at.rag = (any_idle ? 3 : 2) * n_pos;
  at.rag_steps = c.len && any_idle ? at.rag + at.rag_block() : 0;
  sc.h.resize(at.rag + (c.len ? at.rag_block() * (any_idle ? 1 + n_steps : 1) : 0));
  for (size_t i = 0; i < n_pos; ++i) {  // (utils.py:53-59: the '.' rule holds at position == L - 1)
    sc.h[i] = pos[i] == CZC_POS_IDLE && c.from ? CZC_POS_IDLE : c.seed_len + pos[i];
    sc.h[at.dot + i] = pos[i] == (c.len ? c.len[i % B] : c.L) - 1 ? 1 : 0;
  }
  if (any_idle)  // the host knows who runs: every step's rows that are not idle, ascending (the tail of a slice is not read)
    for (int s = 0; s < n_steps; ++s) {
      int32_t* list = sc.h.data() + at.runs(s);
      int n = 0;
      for (int r = 0; r < B; ++r)
        if (pos[(size_t)s * B + r] != CZC_POS_IDLE) list[n++] = r;
      for (; n < B; ++n) list[n] = 0;
    }
  if (c.len) {  // [B] lengths then [B + 1] offsets: of the full batch, then (idle calls) of every step's run list
    int32_t* blk = sc.h.data() + at.rag;
    for (int r = 0; r < B; ++r) {
      blk[r] = c.seed_len + c.len[r] + 1;
      blk[B + r] = at.rag_M;
      at.rag_M += blk[r]; at.rag_max = blk[r] > at.rag_max ? blk[r] : at.rag_max;
    }
    blk[2 * B] = at.rag_M;
    for (int s = 0; s < n_steps && any_idle; ++s) {
      int32_t* sb = sc.h.data() + at.rag_step(s);
      int n = 0, off = 0;
      for (int r = 0; r < B; ++r)
        if (pos[(size_t)s * B + r] != CZC_POS_IDLE) { sb[n] = blk[r]; sb[B + n] = off; off += blk[r]; ++n; }
      sb[B + n] = off;
      for (int i = n; i < B; ++i) { sb[i] = 0; sb[B + i + 1] = off; }
    }
  }
  return sc;
}

// What a rows call leaves in the engine comes back on every exit: no later call may re-use a forward by this call's columns (they
// are the caller's memory), so the set-up and the steps in its scope leave through E_CHECK / E_HIP.  A rows call that fails waits
// for the work it has queued.
struct CallScope {
  czc_engine* e; bool rows, ok = false;
  ~CallScope() {
    if (rows) { e->bert_pruned_rows = nullptr; if (!ok) (void)hipStreamSynchronize(e->st); }
  }
};

// What upload_call leaves for the steps of a call: the start rows, the image rows [R, D] they are scored against (the resident
// batch, or its gather by image_of_row) and the per-row records
struct CallBatch { int* d_inp = nullptr; const float* img = nullptr; RowRecords rec; };

// The uploads of a call: the start rows and, for a rows call, the schedule, the per-row records and the gather of its image rows
static int upload_call(czc_engine* e, RowsCall& c, Sched& sc, CallBatch* cb) {
  const int B = c.R, T = c.T, D = e->cfg.clip_proj;
  cb->img = resident_images(e, B);
  auto put = [e](const char* name, const void* src, size_t bytes, void** out) -> int {
    E_CHECK(ensure(e, name, bytes, out));
    E_HIP(hipMemcpyAsync(*out, src, bytes, hipMemcpyHostToDevice, e->st));
    return 0;
  };
  { int* flag; E_CHECK(ensure(e, "s_nonfinite", 32, (void**)&flag)); E_HIP(hipMemsetAsync(flag, 0, 32, e->st)); }
  if (c.from) {  // every row brings its own start row: one upload, no broadcast
    E_CHECK(put("g_inp", c.init, (size_t)B * T * 4, (void**)&cb->d_inp));
  } else {
    int* d_row;
    E_CHECK(ensure(e, "g_inp", (size_t)B * T * 4, (void**)&cb->d_inp));
    E_CHECK(put("g_row", c.init, (size_t)T * 4, (void**)&d_row));
    E_CHECK(launch_broadcast_rows_i32(d_row, T, B, cb->d_inp, e->st));
  }
  if (!c.rows) return 0;
  RowRecords& rec = cb->rec;  // one record per row, uploaded once with the schedule
  static_assert(sizeof(RowHyper) == sizeof(czc_hyper) && offsetof(RowHyper, temperature) == offsetof(czc_hyper, temperature) &&
                offsetof(RowHyper, control) == offsetof(czc_hyper, control) && offsetof(RowHyper, negative) == offsetof(czc_hyper, negative),
                "RowHyper is czc_hyper as the kernels read it");
  static_assert(sizeof(RowDraw) == sizeof(czc_draw) && offsetof(RowDraw, seed_lo) == offsetof(czc_draw, seed) &&
                offsetof(RowDraw, tau) == offsetof(czc_draw, tau) && offsetof(RowDraw, step0) == offsetof(czc_draw, step0),
                "RowDraw is czc_draw as the kernels read it (little-endian seed halves)");
  if (!sc.h.empty()) E_CHECK(put("g_sched", sc.h.data(), sc.h.size() * 4, (void**)&sc.d));
  if (c.hp_rows) E_CHECK(put("g_hp_rows", c.hp_rows, (size_t)B * sizeof(RowHyper), (void**)&rec.hp));
  if (c.draw) E_CHECK(put("g_draw_rows", c.draw, (size_t)B * sizeof(RowDraw), (void**)&rec.draw));
  if (c.rival) {  // the indices point into the whole resident batch, not into the rows' gather below
    E_CHECK(put("g_rival", c.rival, (size_t)B * c.M * 4, (void**)&rec.rival));
    E_CHECK(put("g_rdelta", c.delta, (size_t)B * 4, (void**)&rec.delta));
    rec.M = c.M; rec.img_all = e->d_img_n; rec.n_img = e->img_B;
  }
  if (c.vset) {  // the whole table of bitsets and an index per row; the top-K kernel of a set call reads its temperature per row
    rec.vwords = (e->cfg.bert_vocab + 31) / 32;
    E_CHECK(put("g_vset", c.vset, (size_t)B * 4, (void**)&rec.vset));
    E_CHECK(put("g_vbits", c.sets, (size_t)c.n_sets * rec.vwords * 4, (void**)&rec.vbits));
    if (!c.hp_rows) {
      c.vocab_hp.assign((size_t)B, *c.hp);
      E_CHECK(put("g_vhp", c.vocab_hp.data(), (size_t)B * sizeof(RowHyper), (void**)&rec.vhp));
    }
  }
  // the embedding of row r is that of image image_of_row[r] -- one gather of the normalised embeds to [R, D] here, and the step
  // sees a batch of R images (what the memo's compact batches do), so no tower or combine kernel changes
  if (c.image_of_row) {
    int* d_ior; float* img_r;
    E_CHECK(ensure(e, "g_img_r", (size_t)B * D * 4, (void**)&img_r));
    E_CHECK(put("g_ior", c.image_of_row, (size_t)B * 4, (void**)&d_ior));
    E_CHECK(launch_gather_rows_f32(e->d_img_n, d_ior, B, D, img_r, e->st));
    cb->img = img_r;
  }
  return 0;
}

// The steps of a call and its snapshots (inside a CallScope, behind upload_call)
static int run_steps(czc_engine* e, const RowsCall& c, const Sched& sc, const CallBatch& cb) {
  int* const d_inp = cb.d_inp;
  const int B = c.R, T = c.T, L = c.L, seed_len = c.seed_len, n_steps = c.n_steps, snapshot_every = c.snapshot_every;
  const bool rows = c.rows;
  float* out_cos = c.out_cos;
  // what this call returns of a step: the ids it leaves in d_inp and, at the snapshot steps, the winner's cosine
  // AUDIT steps -- the snapshot step of every fourth sweep, starting with the first -- take the full selection for every
  // image: there the guard (czc_refine_guard) measures the screening tower on all images although most other steps are
  // gated (a checkpoint the fp16 tower carries badly trips it in the first sweep).  At the other snapshot steps a gated
  // image re-encodes its winner alone, for the cosine this call returns.  The gate is the guard's dependant: with the guard
  // switched off (refine_guard_x1e6 = 0) nothing polices the bound the gate rests on, so nothing is gated
  // (whether or not the caller reads cosines: the guard must see the screening tower on every call -- and a call too short
  // to reach a snapshot step is audited at its last step)
  std::vector<char> audit(n_steps, 0);
  { bool audited = false;
    for (int s = 0; s < n_steps; ++s) {
      const bool snap_idx = (s + 1) % snapshot_every == 0;
      audit[s] = (snap_idx && (s / snapshot_every) % 4 == 0) || (s + 1 == n_steps && !audited);
      audited = audited || audit[s];
    } }
  // The steps whose winner cosine this call returns: the snapshot steps and, in a call with idle steps, every step after which
  // some row sits out the rest of its snapshot interval -- that row's cosine at the snapshot is the one this step leaves, so a
  // gated row re-encodes its winner here as it does at a snapshot step (a row then returns the exact tower's cosine whether
  // or not its companions run longer than it does)
  std::vector<char> cos_step(n_steps, 0);
  if (out_cos) {
    std::vector<char> later(rows && sc.at.idle ? B : 0, 1);  // the row runs again before the coming snapshot (none comes: nothing is returned)
    for (int s = n_steps - 1; s >= 0; --s) {
      const bool snap_idx = (s + 1) % snapshot_every == 0;
      cos_step[s] = snap_idx;
      if (snap_idx) std::fill(later.begin(), later.end(), 0);
      for (size_t r = 0; r < later.size(); ++r)
        if (c.positions[(size_t)s * B + r] != CZC_POS_IDLE) { cos_step[s] = cos_step[s] || !later[r]; later[r] = 1; }
    }
  }
  MemoPlan mp;
  const bool memo = e->memo && !rows;  // the memo's keys are (image, position, n_mask); a rows call has option "memo_rows"
  if (memo) E_CHECK(memo_begin(e, c, audit, &mp));
  MemoRowsPlan mrp;
  const bool memo_rows = rows && (e->memo_rows || sc.at.idle) && n_steps > 0;  // the compact-batch path, with or without entries
  if (memo_rows) E_CHECK(memo_rows_begin(e, c, audit, &mrp));
  Ragged rag_full{};
  if (c.len && sc.d) {
    rag_full = Ragged{sc.d + sc.at.rag + B, sc.d + sc.at.rag, sc.at.rag_M, sc.at.rag_max};
    if (memo_rows) {
      mrp.len_h = sc.h.data() + sc.at.rag;
      E_CHECK(ensure(e, "mr_rag_c", sc.at.rag_block() * 4, (void**)&mrp.d_rag_c));
    }
  }
  if (memo_rows && cb.rec.hp) E_CHECK(ensure(e, "mr_hp_c", (size_t)B * sizeof(RowHyper), (void**)&mrp.rec_c.hp));
  if (memo_rows && cb.rec.draw) E_CHECK(ensure(e, "mr_draw_c", (size_t)B * sizeof(RowDraw), (void**)&mrp.rec_c.draw));
  if (memo_rows && cb.rec.rival) {
    E_CHECK(ensure(e, "mr_riv_c", (size_t)B * c.M * 4, (void**)&mrp.rec_c.rival));
    E_CHECK(ensure(e, "mr_rdelta_c", (size_t)B * 4, (void**)&mrp.rec_c.delta));
  }
  if (memo_rows && cb.rec.vset) E_CHECK(ensure(e, "mr_vset_c", (size_t)B * 4, (void**)&mrp.rec_c.vset));
  // czc_generate_rows_tied (check_groups has run): the group table goes up once, behind the schedule
  TiePlan tie;
  const bool tied = c.group != nullptr && n_steps > 0;
  if (tied) E_CHECK(tie_begin(e, B, T, seed_len, c.group, c.len, out_cos != nullptr, &tie));
  // a row that has not run yet in this call reports cosine 0 (the reference's best_clip_score start value)
  if (memo_rows && sc.at.idle && hipMemsetAsync(mrp.bcos, 0, (size_t)B * 4, e->st) != hipSuccess)
    return fail(e, CZC_ERR_HIP, "generate_rows_from: clearing the cosines%s");
  int snap = 0;
  StepOut so;  // of the step that ran on the whole batch, without a memo
  for (int s = 0; s < n_steps; ++s) {
    const int pos = c.positions[rows ? (size_t)s * B : (size_t)s];
    const int nm = c.n_mask_at(s), dot = pos == L - 1 ? 1 : 0;
    const bool snap_idx = (s + 1) % snapshot_every == 0;
    StepArgs a{d_inp, B, T, seed_len + pos, nm, dot, c.top_k, *c.hp};  // (rows: row 0's column and '.' rule)
    a.img = cb.img; a.rec = cb.rec; a.rec.step = (unsigned)s;
    a.mode = StepMode{true, e->refine && e->refine_gate_delta > 0.f && e->refine_guard_dev > 0.f && !audit[s], cos_step[s] != 0};
    if (rows) {
      a.gen_rows = sc.d + sc.at.cols(s); a.dot_rows = sc.d + sc.at.dots(s); a.gen_rows_host = sc.h.data() + sc.at.cols(s);
      a.rag = c.len ? &rag_full : nullptr;
      a.ctl_T = c.len ? seed_len + c.len[0] + 1 : 0;  // (a callback call's rows share one length: checked above)
    }
    if (memo_rows) E_CHECK(memo_rows_step(e, mrp, c, sc, s, a));
    else if (memo) E_CHECK(memo_step(e, mp, s, a));
    else E_CHECK(step_device(e, a, &so));
    // the tie: one launch on the full batch, behind whatever the step did (in place, compact batch and scatter, memo fill)
    if (tied && launch_tie_rows(d_inp, B, T, sc.d + sc.at.cols(s), tie.d_gor, tie.d_off, tie.d_rows, e->st)) return fail(e, CZC_ERR_HIP, "%s", g_err);
    // a tied call returns the cosine of the caption as it stands, one score per group
    if (tied && snap_idx && out_cos) E_CHECK(tie_score(e, tie, d_inp, cb.img, B, T, c.len != nullptr));
    if (snap_idx) {
      hipError_t h = c.out_ids ? hipMemcpyAsync(c.out_ids + (size_t)snap * B * T, d_inp, (size_t)B * T * 4, hipMemcpyDefault, e->st) : hipSuccess;
      if (out_cos && h == hipSuccess)  // memo: the full-batch cosines (a compacted step leaves B_act of them in s_bcos)
        h = hipMemcpyAsync(out_cos + (size_t)snap * B, tied ? tie.cos : memo ? mp.bcos : memo_rows ? mrp.bcos : so.bcos, (size_t)B * 4,
                           hipMemcpyDefault, e->st);
      if (h != hipSuccess) { snprintf(e->err, sizeof(e->err), "generate: snapshot copy -> %s", hipGetErrorString(h)); return CZC_ERR_HIP; }
      ++snap;
    }
  }
  return 0;
}

static int generate_impl(czc_engine* e, RowsCall& c) {
  bool any_idle = false;
  if (int rc = check_call(e, c, &any_idle)) return rc;
  Sched sc = build_schedule(c, any_idle);
  { CallScope scope{e, c.rows};
    CallBatch cb;
    E_CHECK(upload_call(e, c, sc, &cb));
    E_CHECK(run_steps(e, c, sc, cb));
    scope.ok = true; }
  return finish_steps(e);
}

// ---- the checks of the optional per-row arrays: each validates its array and, where the array carries nothing, drops it, so
// that the call underneath is the simpler one, bit for bit

// len (czc_generate_rows_len and above): rows of one length that fill the stride are czc_generate_rows_from itself
static int check_lengths(czc_engine* e, RowsCall& c) {
  const int R = c.R, T = c.T, seed_len = c.seed_len;
  if (!e || !c.init || !c.len || !c.positions || !c.hp || R <= 0 || c.n_steps < 0 || c.snapshot_every <= 0)
    return CZC_ERR_ARG;
  e->err[0] = 0;
  if (R > CZC_MAX_ROWS || seed_len < 0 || T > CZC_MAX_BERT_LEN) return fail(e, CZC_ERR_ARG, "generate_rows_len: R > CZC_MAX_ROWS, seed_len < 0 or T > CZC_MAX_BERT_LEN%s");
  bool uniform = true;
  int L_max = 0;
  for (int r = 0; r < R; ++r) {
    const int Lr = c.len[r];
    if (Lr < 1 || Lr > T - seed_len - 1) return fail(e, CZC_ERR_ARG, "generate_rows_len: len_of_row outside [1, T - seed_len - 1]%s");
    uniform = uniform && seed_len + Lr + 1 == T;
    L_max = Lr > L_max ? Lr : L_max;
    for (int t = seed_len + Lr + 1; t < T; ++t)
      if (c.init[(size_t)r * T + t] != 0) return fail(e, CZC_ERR_ARG, "generate_rows_len: the columns behind a row's seed_len + len_of_row + 1 tokens must hold id 0 ([PAD])%s");
  }
  for (int s = 0; s < c.n_steps; ++s) {
    const int nm = c.n_mask_at(s);
    for (int r = 0; r < R; ++r) {
      const int p = c.positions[(size_t)s * R + r];
      if (p < CZC_POS_IDLE || p >= c.len[r]) return fail(e, CZC_ERR_ARG, "generate_rows_len: position outside {CZC_POS_IDLE} and [0, len_of_row[r])%s");
      if (p >= 0 && nm > 1 && p + nm > c.len[r])
        return fail(e, CZC_ERR_ARG, "generate_rows_len: an n_mask >= 2 step masks past the row's last position (it needs position + n_mask <= len_of_row[r])%s");
    }
  }
  c.L = L_max;
  if (uniform) c.len = nullptr;
  return 0;
}

// hp_rows (czc_generate_rows_hp and above): equal entries are the scalar call with entry 0 (its scalar kernels)
static int check_hypers(czc_engine* e, RowsCall& c) {
  const int R = c.R;
  if (!e || !c.init || !c.positions || !c.hp_rows || R <= 0 || c.n_steps < 0 || c.snapshot_every <= 0) return CZC_ERR_ARG;
  e->err[0] = 0;
  if (R > CZC_MAX_ROWS) return fail(e, CZC_ERR_ARG, "generate_rows_hp: R > CZC_MAX_ROWS%s");
  bool uniform = true, any_ctl = false, one_signal = true;
  for (int r = 0; r < R; ++r) {
    const czc_hyper& h = c.hp_rows[r];
    if (h.control < 0 || h.control > 2) return fail(e, CZC_ERR_ARG, "generate_rows_hp: control outside {0, 1, 2}%s");
    if (!std::isfinite(h.temperature) || !(h.temperature > 0.f)) return fail(e, CZC_ERR_ARG, "generate_rows_hp: a temperature must be finite and > 0%s");
    if (!std::isfinite(h.alpha) || !std::isfinite(h.beta) || !std::isfinite(h.gamma)) return fail(e, CZC_ERR_ARG, "generate_rows_hp: alpha, beta and gamma must be finite%s");
    uniform = uniform && memcmp(&h, &c.hp_rows[0], sizeof(czc_hyper)) == 0;
    any_ctl = any_ctl || h.control != 0;
    one_signal = one_signal && h.control == c.hp_rows[0].control && (h.negative != 0) == (c.hp_rows[0].negative != 0);
  }
  // the host scorer is configured for one signal, and it is called for every row of a controlled step
  if (e->ctl_fn && any_ctl && !one_signal)
    return fail(e, CZC_ERR_ARG, "generate_rows_hp: a control callback scores one signal, so every row must share control and negative; "
                                "use the control tables (czc_set_lexicon / czc_set_lexicon_pos / czc_set_pos)%s");
  for (int r = 0; r < R; ++r) {  // step_device's messages, before any GPU work
    if (c.hp_rows[r].control == 1 && !e->ctl_fn && !e->d_lex && !e->d_lex_pos)
      return fail(e, CZC_ERR_STATE, "sentiment path needs a lexicon (czc_set_lexicon / czc_set_lexicon_pos) or czc_set_control_callback%s");
    if (c.hp_rows[r].control == 2 && !e->ctl_fn && !e->d_pos_tags)
      return fail(e, CZC_ERR_STATE, "POS path needs czc_set_pos or czc_set_control_callback%s");
  }
  c.hp = &c.hp_rows[0];
  if (uniform && !c.rival) c.hp_rows = nullptr;  // (a rival call always carries its records)
  return 0;
}

// draw (czc_generate_rows_draw and above; may be null): no row with tau > 0 is czc_generate_rows_hp itself
static int check_draws(czc_engine* e, RowsCall& c) {
  if (!e || c.R <= 0 || c.n_steps < 0) return CZC_ERR_ARG;
  e->err[0] = 0;
  if (c.R > CZC_MAX_ROWS) return fail(e, CZC_ERR_ARG, "generate_rows_draw: R > CZC_MAX_ROWS%s");
  bool any = false;
  for (int r = 0; r < c.R && c.draw; ++r) {
    const czc_draw& d = c.draw[r];
    if (!std::isfinite(d.tau) || d.tau < 0.f) return fail(e, CZC_ERR_ARG, "generate_rows_draw: a tau must be finite and >= 0%s");
    if ((uint64_t)d.step0 + (uint64_t)c.n_steps > 0xffffffffull)
      return fail(e, CZC_ERR_ARG, "generate_rows_draw: step0 + n_steps does not fit the 32-bit step counter%s");
    any = any || d.tau > 0.f;
  }
  if (!any && !c.rival) c.draw = nullptr;  // (a rival call always carries its records)
  return 0;
}

// group (czc_generate_rows_tied and above, not null): rows tied into groups that hold one sentence
static int check_groups(czc_engine* e, const RowsCall& c) {
  const int R = c.R, T = c.T;
  if (!e || !c.init || !c.positions || R <= 0 || c.n_steps < 0) return CZC_ERR_ARG;
  e->err[0] = 0;
  if (R > CZC_MAX_ROWS || c.seed_len < 0 || T <= 0 || T > CZC_MAX_BERT_LEN) return fail(e, CZC_ERR_ARG, "generate_rows_tied: R > CZC_MAX_ROWS, seed_len < 0 or T outside [1, CZC_MAX_BERT_LEN]%s");
  for (int s = 0; s < c.n_steps && c.n_mask; ++s)
    if (c.n_mask[s] != 1) return fail(e, CZC_ERR_ARG, "generate_rows_tied: every step needs n_mask = 1 (the n_mask = 0 re-use of a forward across a tie is not defined; span order is refused)%s");
  std::vector<int32_t> lead(R, -1);  // by group id: its lowest-numbered row
  for (int r = 0; r < R; ++r) {
    const int g = c.group[r];
    if (g < 0 || g >= R) return fail(e, CZC_ERR_ARG, "generate_rows_tied: a group id outside [0, R)%s");
    if (lead[g] < 0) { lead[g] = r; continue; }
    const int l = lead[g];
    if (c.len && c.len[r] != c.len[l])
      return fail(e, CZC_ERR_ARG, "generate_rows_tied: the rows of a group must share one length%s");
    if (c.image_of_row ? c.image_of_row[r] != c.image_of_row[l] : true)  // (image_of_row = NULL: row r has image r)
      return fail(e, CZC_ERR_ARG, "generate_rows_tied: the rows of a group must share one image%s");
    if (memcmp(c.init + (size_t)r * T, c.init + (size_t)l * T, (size_t)T * 4) != 0)
      return fail(e, CZC_ERR_ARG, "generate_rows_tied: the rows of a group must bring the same start row%s");
  }
  std::vector<int32_t> seen((size_t)R * T, -1);  // (group, position) -> the last step a member ran there
  for (int s = 0; s < c.n_steps; ++s)
    for (int r = 0; r < R; ++r) {
      const int p = c.positions[(size_t)s * R + r];
      if (p < 0 || p >= T) continue;  // idle; anything else out of range is refused by the call's own checks
      int32_t& was = seen[(size_t)c.group[r] * T + p];
      if (was == s) return fail(e, CZC_ERR_ARG, "generate_rows_tied: two rows of a group run at the same position in one step%s");
      was = s;
    }
  return 0;
}

// the checks of a rival table, shared by czc_generate_rows_vs and czc_score_rows_vs (image_of_row and R are checked by then);
// *active: some row has a filled slot (and, with deltas, a delta != 0)
static int check_rivals(czc_engine* e, const char* who, int R, const int32_t* image_of_row_host, const int32_t* rival, int M,
                        const float* delta, bool* active) {
  static_assert(czc::CB_MAX_RIVALS == CZC_MAX_RIVALS, "the kernels' rival slots are the header's");
  *active = false;
  if (M < 1 || M > CZC_MAX_RIVALS) return fail(e, CZC_ERR_ARG, "%s: M outside [1, CZC_MAX_RIVALS]", who);
  if ((size_t)e->cfg.clip_proj * CZC_MAX_RIVALS * 4 > (size_t)czc::CB_RIVAL_FLOATS * 4)
    return fail(e, CZC_ERR_ARG, "%s: clip_proj * CZC_MAX_RIVALS * 4 exceeds the rival kernel's LDS array (32 KB)", who);
  for (int r = 0; r < R; ++r) {
    if (delta && !std::isfinite(delta[r])) return fail(e, CZC_ERR_ARG, "%s: a delta must be finite", who);
    const int own = image_of_row_host ? image_of_row_host[r] : r;
    bool empty = false;
    for (int j = 0; j < M; ++j) {
      const int v = rival[(size_t)r * M + j];
      if (v < -1 || v >= e->img_B) return fail(e, CZC_ERR_ARG, "%s: a rival index outside [-1, resident image batch)", who);
      if (v == -1) { empty = true; continue; }
      if (empty) return fail(e, CZC_ERR_ARG, "%s: a filled rival slot behind an empty one (the filled slots come first)", who);
      if (v == own) return fail(e, CZC_ERR_ARG, "%s: a rival equal to the row's own image", who);
    }
    if (rival[(size_t)r * M] >= 0 && (!delta || delta[r] != 0.f)) *active = true;
  }
  return 0;
}

// rival + delta (czc_generate_rows_vs, rival not null): no row with both a rival and a delta is czc_generate_rows_tied itself.
// A call that keeps its table always carries per-row records: rows without a draw record keep the first argmax (tau = 0)
static int check_rival_table(czc_engine* e, RowsCall& c) {
  const int R = c.R;
  if (!e || R <= 0 || !c.delta) return CZC_ERR_ARG;
  e->err[0] = 0;
  if (R > CZC_MAX_ROWS) return fail(e, CZC_ERR_ARG, "generate_rows_vs: R > CZC_MAX_ROWS%s");
  if (!e->d_img_n || e->img_B <= 0) return fail(e, CZC_ERR_STATE, "image embeds not set%s");
  if (!c.image_of_row && e->img_B != R) return fail(e, CZC_ERR_ARG, "generate_rows_vs: image_of_row = NULL needs R equal to the resident image batch%s");
  for (int r = 0; r < R && c.image_of_row; ++r)
    if (c.image_of_row[r] < 0 || c.image_of_row[r] >= e->img_B)
      return fail(e, CZC_ERR_ARG, "generate_rows_vs: image_of_row outside the resident image batch%s");
  bool active = false;
  E_CHECK(check_rivals(e, "generate_rows_vs", R, c.image_of_row, c.rival, c.M, c.delta, &active));
  if (!active) { c.rival = nullptr; return 0; }
  if (e->refine)
    return fail(e, CZC_ERR_STATE, "generate_rows_vs: the selection and guard bounds of CZC_PREC_REFINE were derived for the softmax-K term alone; "
                                  "run rows with rivals on a CZC_PREC_SPLIT engine%s");
  if (!c.draw) { c.no_draw.assign((size_t)R, czc_draw{0, 0.f, 0}); c.draw = c.no_draw.data(); }
  return 0;
}

// sets + vset (czc_generate_rows_vocab, vset not null): no row with a set is czc_generate_rows_vs itself
static int check_vocab(czc_engine* e, RowsCall& c) {
  if (!e || c.R <= 0) return CZC_ERR_ARG;
  e->err[0] = 0;
  if (c.R > CZC_MAX_ROWS) return fail(e, CZC_ERR_ARG, "generate_rows_vocab: R > CZC_MAX_ROWS%s");
  if (c.n_sets < 1) return fail(e, CZC_ERR_ARG, "generate_rows_vocab: n_sets < 1 with a set_of_row array%s");
  if (c.n_sets > CZC_MAX_VOCAB_SETS) return fail(e, CZC_ERR_ARG, "generate_rows_vocab: n_sets > CZC_MAX_VOCAB_SETS%s");
  bool any = false;
  for (int r = 0; r < c.R; ++r) {
    if (c.vset[r] < -1 || c.vset[r] >= c.n_sets) return fail(e, CZC_ERR_ARG, "generate_rows_vocab: a set_of_row index outside [-1, n_sets)%s");
    any = any || c.vset[r] >= 0;
  }
  if (any && !c.sets) return fail(e, CZC_ERR_ARG, "generate_rows_vocab: sets is NULL and a set_of_row index is >= 0%s");
  if (!any) c.vset = nullptr;
  return 0;
}

// The driver: the checks of the arrays the entry point has, outermost argument first, then the call itself
static int run_call(czc_engine* e, RowsCall& c) {
  int rc = 0;
  if (c.level >= CALL_VOCAB && c.vset && (rc = check_vocab(e, c))) return rc;
  if (c.level >= CALL_VS && c.rival && (rc = check_rival_table(e, c))) return rc;
  if (c.level >= CALL_TIED && c.group && (rc = check_groups(e, c))) return rc;
  if (c.level >= CALL_DRAW && (rc = check_draws(e, c))) return rc;
  if (c.level >= CALL_HP && (rc = check_hypers(e, c))) return rc;
  if (c.level >= CALL_LEN && (c.len || c.level == CALL_LEN)) { if ((rc = check_lengths(e, c))) return rc; }
  else if (c.level >= CALL_HP) c.L = c.T - c.seed_len - 1;  // lens = NULL: the shape of czc_generate_rows_from
  return generate_impl(e, c);
}

static RowsCall new_call(CallLevel level, int R, int T, int seed_len, int top_k, int n_steps, int snapshot_every, int32_t* out_ids, float* out_cos) {
  RowsCall c;
  c.level = level; c.rows = level >= CALL_ROWS; c.from = level >= CALL_FROM; c.out_ids = out_ids; c.out_cos = out_cos;
  c.R = R; c.T = T; c.seed_len = seed_len; c.top_k = top_k; c.n_steps = n_steps; c.snapshot_every = snapshot_every;
  return c;
}

int czc_generate(czc_engine* e, int B, int T, int L, int seed_len, const int32_t* init_ids_host, int top_k,
                 int n_steps, const int32_t* positions_host, const int32_t* n_mask_host, int snapshot_every,
                 const czc_hyper* hp, int32_t* out_ids, float* out_cos) {
  RowsCall c = new_call(CALL_GENERATE, B, T, seed_len, top_k, n_steps, snapshot_every, out_ids, out_cos);
  c.L = L; c.init = init_ids_host; c.positions = positions_host; c.n_mask = n_mask_host; c.hp = hp;
  return run_call(e, c);
}

int czc_generate_rows(czc_engine* e, int R, int T, int L, int seed_len, const int32_t* init_ids_host,
                      const int32_t* image_of_row_host, int top_k, int n_steps, const int32_t* positions_host,
                      const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp, int32_t* out_ids, float* out_cos) {
  RowsCall c = new_call(CALL_ROWS, R, T, seed_len, top_k, n_steps, snapshot_every, out_ids, out_cos);
  c.L = L; c.init = init_ids_host; c.image_of_row = image_of_row_host; c.positions = positions_host; c.n_mask = n_mask_host; c.hp = hp;
  return run_call(e, c);
}

int czc_generate_rows_from(czc_engine* e, int R, int T, int L, int seed_len, const int32_t* init_rows_host,
                           const int32_t* image_of_row_host, int top_k, int n_steps, const int32_t* positions_host,
                           const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp, int32_t* out_ids, float* out_cos) {
  RowsCall c = new_call(CALL_FROM, R, T, seed_len, top_k, n_steps, snapshot_every, out_ids, out_cos);
  c.L = L; c.init = init_rows_host; c.image_of_row = image_of_row_host; c.positions = positions_host; c.n_mask = n_mask_host; c.hp = hp;
  return run_call(e, c);
}

int czc_generate_rows_len(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host, const int32_t* len_of_row_host,
                          const int32_t* image_of_row_host, int top_k, int n_steps, const int32_t* positions_host,
                          const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp, int32_t* out_ids, float* out_cos) {
  RowsCall c = new_call(CALL_LEN, R, T, seed_len, top_k, n_steps, snapshot_every, out_ids, out_cos);
  c.init = init_rows_host; c.len = len_of_row_host; c.image_of_row = image_of_row_host; c.positions = positions_host; c.n_mask = n_mask_host; c.hp = hp;
  return run_call(e, c);
}

int czc_generate_rows_hp(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host, const int32_t* len_of_row_host,
                         const int32_t* image_of_row_host, int top_k, int n_steps, const int32_t* positions_host,
                         const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp_of_row_host, int32_t* out_ids, float* out_cos) {
  RowsCall c = new_call(CALL_HP, R, T, seed_len, top_k, n_steps, snapshot_every, out_ids, out_cos);
  c.init = init_rows_host; c.len = len_of_row_host; c.image_of_row = image_of_row_host; c.positions = positions_host; c.n_mask = n_mask_host;
  c.hp_rows = hp_of_row_host;
  return run_call(e, c);
}

int czc_generate_rows_draw(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host, const int32_t* len_of_row_host,
                           const int32_t* image_of_row_host, int top_k, int n_steps, const int32_t* positions_host,
                           const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp_of_row_host,
                           const czc_draw* draw_of_row_host, int32_t* out_ids, float* out_cos) {
  RowsCall c = new_call(CALL_DRAW, R, T, seed_len, top_k, n_steps, snapshot_every, out_ids, out_cos);
  c.init = init_rows_host; c.len = len_of_row_host; c.image_of_row = image_of_row_host; c.positions = positions_host; c.n_mask = n_mask_host;
  c.hp_rows = hp_of_row_host; c.draw = draw_of_row_host;
  return run_call(e, c);
}

int czc_generate_rows_tied(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host, const int32_t* len_of_row_host,
                           const int32_t* image_of_row_host, const int32_t* group_of_row_host, int top_k, int n_steps,
                           const int32_t* positions_host, const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp_of_row_host,
                           const czc_draw* draw_of_row_host, int32_t* out_ids, float* out_cos) {
  RowsCall c = new_call(CALL_TIED, R, T, seed_len, top_k, n_steps, snapshot_every, out_ids, out_cos);
  c.init = init_rows_host; c.len = len_of_row_host; c.image_of_row = image_of_row_host; c.positions = positions_host; c.n_mask = n_mask_host;
  c.hp_rows = hp_of_row_host; c.draw = draw_of_row_host; c.group = group_of_row_host;
  return run_call(e, c);
}

int czc_generate_rows_vs(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host, const int32_t* len_of_row_host,
                         const int32_t* image_of_row_host, const int32_t* group_of_row_host, int top_k, int n_steps,
                         const int32_t* positions_host, const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp_of_row_host,
                         const czc_draw* draw_of_row_host, const int32_t* rival_of_row_host, int M, const float* delta_of_row_host,
                         int32_t* out_ids, float* out_cos) {
  RowsCall c = new_call(CALL_VS, R, T, seed_len, top_k, n_steps, snapshot_every, out_ids, out_cos);
  c.init = init_rows_host; c.len = len_of_row_host; c.image_of_row = image_of_row_host; c.positions = positions_host; c.n_mask = n_mask_host;
  c.hp_rows = hp_of_row_host; c.draw = draw_of_row_host; c.group = group_of_row_host; c.rival = rival_of_row_host; c.M = M; c.delta = delta_of_row_host;
  return run_call(e, c);
}

int czc_generate_rows_vocab(czc_engine* e, int R, int T, int seed_len, const int32_t* init_rows_host, const int32_t* len_of_row_host,
                            const int32_t* image_of_row_host, const int32_t* group_of_row_host, int top_k, int n_steps,
                            const int32_t* positions_host, const int32_t* n_mask_host, int snapshot_every, const czc_hyper* hp_of_row_host,
                            const czc_draw* draw_of_row_host, const int32_t* rival_of_row_host, int M, const float* delta_of_row_host,
                            const uint32_t* sets_host, int n_sets, const int32_t* set_of_row_host, int32_t* out_ids, float* out_cos) {
  RowsCall c = new_call(CALL_VOCAB, R, T, seed_len, top_k, n_steps, snapshot_every, out_ids, out_cos);
  c.init = init_rows_host; c.len = len_of_row_host; c.image_of_row = image_of_row_host; c.positions = positions_host; c.n_mask = n_mask_host;
  c.hp_rows = hp_of_row_host; c.draw = draw_of_row_host; c.group = group_of_row_host; c.rival = rival_of_row_host; c.M = M; c.delta = delta_of_row_host;
  c.sets = sets_host; c.n_sets = n_sets; c.vset = set_of_row_host;
  return run_call(e, c);
}

static int score_rows_impl(czc_engine* e, const char* who, const int32_t* rows, int R, int T, int seed_len, const int32_t* len_of_row_host,
                           const int32_t* image_of_row_host, const int32_t* rival_of_row_host, int M, float* out_cos, float* out_disc);

int czc_score_rows(czc_engine* e, const int32_t* rows, int R, int T, int seed_len, const int32_t* len_of_row_host,
                   const int32_t* image_of_row_host, float* out_cos) {
  if (!out_cos) return CZC_ERR_ARG;
  return score_rows_impl(e, "score_rows", rows, R, T, seed_len, len_of_row_host, image_of_row_host, nullptr, 0, out_cos, nullptr);
}

int czc_score_rows_vs(czc_engine* e, const int32_t* rows, int R, int T, int seed_len, const int32_t* len_of_row_host,
                      const int32_t* image_of_row_host, const int32_t* rival_of_row_host, int M, float* out_cos, float* out_disc) {
  return score_rows_impl(e, "score_rows_vs", rows, R, T, seed_len, len_of_row_host, image_of_row_host, rival_of_row_host, M, out_cos, out_disc);
}

static int score_rows_impl(czc_engine* e, const char* who, const int32_t* rows, int R, int T, int seed_len, const int32_t* len_of_row_host,
                           const int32_t* image_of_row_host, const int32_t* rival_of_row_host, int M, float* out_cos, float* out_disc) {
  if (!e || !rows || R <= 0) return CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  e->err[0] = 0;
  if (R > CZC_MAX_ROWS || seed_len < 0 || T <= 0 || T > CZC_MAX_BERT_LEN) return fail(e, CZC_ERR_ARG, "score_rows: R > CZC_MAX_ROWS, seed_len < 0 or T outside [1, CZC_MAX_BERT_LEN]%s");
  if (!e->finalized) return fail(e, CZC_ERR_STATE, "weights not finalized%s");
  if (!e->has_bridge) return fail(e, CZC_ERR_STATE, "bridge tables not set%s");
  if (!e->d_img_n || e->img_B <= 0) return fail(e, CZC_ERR_STATE, "image embeds not set%s");
  if (!image_of_row_host && e->img_B != R) return fail(e, CZC_ERR_ARG, "score_rows: image_of_row = NULL needs R equal to the resident image batch%s");
  for (int r = 0; r < R; ++r) {
    if (image_of_row_host && (image_of_row_host[r] < 0 || image_of_row_host[r] >= e->img_B))
      return fail(e, CZC_ERR_ARG, "score_rows: image_of_row outside the resident image batch%s");
    if (len_of_row_host && (len_of_row_host[r] < 1 || len_of_row_host[r] > T - seed_len - 1))
      return fail(e, CZC_ERR_ARG, "score_rows: len_of_row outside [1, T - seed_len - 1]%s");
  }
  bool any_rival = false;
  if (rival_of_row_host) E_CHECK(check_rivals(e, who, R, image_of_row_host, rival_of_row_host, M, nullptr, &any_rival));
  const size_t n = (size_t)R * T;
  std::vector<int32_t> host;
  const int32_t* h = rows;
  const bool on_device = is_device_ptr(rows);
  if (on_device) {  // the ids are checked on the host either way: they index the bridge tables
    host.resize(n);
    E_HIP(hipMemcpyAsync(host.data(), rows, n * 4, hipMemcpyDeviceToHost, e->st));
    E_HIP(hipStreamSynchronize(e->st));
    h = host.data();
  }
  for (int r = 0; r < R; ++r) {
    const int Tr = len_of_row_host ? seed_len + len_of_row_host[r] + 1 : T;
    for (int t = 0; t < Tr; ++t)
      if (h[(size_t)r * T + t] < 0 || h[(size_t)r * T + t] >= e->cfg.bert_vocab)
        return fail(e, CZC_ERR_ARG, "score_rows: a row holds an id outside the BERT vocabulary%s");
  }
  const int D = e->cfg.clip_proj;
  int *d_rows, *d_len = nullptr, *d_ior; float *img_r = e->d_img_n, *d_cos;
  { int* flag; E_CHECK(ensure(e, "s_nonfinite", 32, (void**)&flag)); E_HIP(hipMemsetAsync(flag, 0, 32, e->st)); }
  E_CHECK(ensure(e, "sc_rows", n * 4, (void**)&d_rows));
  E_CHECK(ensure(e, "sc_cos", (size_t)R * 4, (void**)&d_cos));
  E_HIP(hipMemcpyAsync(d_rows, rows, n * 4, hipMemcpyDefault, e->st));
  std::vector<int32_t> len_t;
  if (len_of_row_host) {
    len_t.resize(R);
    for (int r = 0; r < R; ++r) len_t[r] = seed_len + len_of_row_host[r] + 1;
    E_CHECK(ensure(e, "sc_len", (size_t)R * 4, (void**)&d_len));
    E_HIP(hipMemcpyAsync(d_len, len_t.data(), (size_t)R * 4, hipMemcpyHostToDevice, e->st));
  }
  if (image_of_row_host) {
    E_CHECK(ensure(e, "sc_ior", (size_t)R * 4, (void**)&d_ior));
    E_CHECK(ensure(e, "sc_img_r", (size_t)R * D * 4, (void**)&img_r));
    E_HIP(hipMemcpyAsync(d_ior, image_of_row_host, (size_t)R * 4, hipMemcpyHostToDevice, e->st));
    E_CHECK(launch_gather_rows_f32(e->d_img_n, d_ior, R, D, img_r, e->st));
  }
  int* d_rival = nullptr; float* d_disc = nullptr;
  if (rival_of_row_host) {
    E_CHECK(ensure(e, "sc_rival", (size_t)R * M * 4, (void**)&d_rival));
    E_CHECK(ensure(e, "sc_disc", (size_t)R * 4, (void**)&d_disc));
    E_HIP(hipMemcpyAsync(d_rival, rival_of_row_host, (size_t)R * M * 4, hipMemcpyHostToDevice, e->st));
  }
  E_CHECK(score_rows_device(e, d_rows, R, T, d_len, img_r, d_cos, d_rival, M, d_disc));  // (its size read waits for the pageable uploads above)
  if (out_cos) E_HIP(hipMemcpyAsync(out_cos, d_cos, (size_t)R * 4, hipMemcpyDefault, e->st));
  if (out_disc && d_disc) E_HIP(hipMemcpyAsync(out_disc, d_disc, (size_t)R * 4, hipMemcpyDefault, e->st));
  if (out_disc && !d_disc)
    for (int r = 0; r < R; ++r) out_disc[r] = 1.0f;  // no table: no row has a rival
  E_HIP(hipMemcpyAsync(e->h_totals + HT_FLAGS, e->ws["s_nonfinite"].p, 4, hipMemcpyDeviceToHost, e->st));
  E_HIP(hipStreamSynchronize(e->st));
  if (e->h_totals[HT_FLAGS]) return fail(e, CZC_ERR_OVERFLOW, MSG_NONFINITE);
  return CZC_OK;
}

// BERT's pseudo-log-likelihood of finished rows (fluency.hip).  The N = sum L_r masked sequences go through bert_forward and
// mlm_head in chunks of at most fluency_chunk, as the sequences of a rows step do (one kept row each, ragged where the rows
// differ in length); the tables of the whole call are uploaded once and nothing is read back before the end.
int czc_fluency_rows(czc_engine* e, const int32_t* rows, int R, int T, int seed_len, const int32_t* len_of_row_host, float temperature,
                     float* out_logp, int32_t* out_rank, float* out_pll) {
  if (!e || !rows) return CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  e->err[0] = 0;
  if (R < 1 || R > CZC_MAX_ROWS || T < 1 || T > CZC_MAX_BERT_LEN || seed_len < 0 || T - seed_len - 1 < 1)
    return fail(e, CZC_ERR_ARG, "fluency_rows: R outside [1, CZC_MAX_ROWS], T outside [1, CZC_MAX_BERT_LEN], seed_len < 0 or T - seed_len - 1 < 1%s");
  if (!out_logp && !out_rank && !out_pll) return fail(e, CZC_ERR_ARG, "fluency_rows: every output is NULL%s");
  if (!std::isfinite(temperature) || !(temperature > 0.f)) return fail(e, CZC_ERR_ARG, "fluency_rows: temperature must be finite and > 0%s");
  const czc_config& c = e->cfg;
  const int Lmax = T - seed_len - 1, V = c.bert_vocab;
  bool dense = true;
  if (len_of_row_host)
    for (int r = 0; r < R; ++r) {
      if (len_of_row_host[r] < 1 || len_of_row_host[r] > Lmax) return fail(e, CZC_ERR_ARG, "fluency_rows: len_of_row outside [1, T - seed_len - 1]%s");
      dense = dense && len_of_row_host[r] == Lmax;
    }
  if (!e->finalized) return fail(e, CZC_ERR_STATE, "weights not finalized%s");
  if (c.bert_layers <= 0) return fail(e, CZC_ERR_STATE, "this engine was created without the BERT tower%s");
  const size_t n_ids = (size_t)R * T;
  std::vector<int32_t> host;
  const int32_t* h = rows;
  if (is_device_ptr(rows)) {  // the ids are checked on the host either way: they index the embedding table
    host.resize(n_ids);
    E_HIP(hipMemcpyAsync(host.data(), rows, n_ids * 4, hipMemcpyDeviceToHost, e->st));
    E_HIP(hipStreamSynchronize(e->st));
    h = host.data();
  }
  for (int r = 0; r < R; ++r) {
    const int Tr = len_of_row_host ? seed_len + len_of_row_host[r] + 1 : T;
    for (int t = 0; t < Tr; ++t)
      if (h[(size_t)r * T + t] < 0 || h[(size_t)r * T + t] >= V) return fail(e, CZC_ERR_ARG, "fluency_rows: a row holds an id outside the BERT vocabulary%s");
  }
  // the tables of the call, one upload: [row_of_seq N][col_of_seq N][out_idx N][seq_len N][seq_off N + n_chunk][len_of_row R]
  // (seq_off: the packed-row offsets of every chunk, each chunk's own exclusive scan starting at 0)
  std::vector<int32_t> tab((size_t)R * Lmax * 2);
  const int N = fluency_expand_tables(R, seed_len, Lmax, len_of_row_host, tab.data(), tab.data() + (size_t)R * Lmax);
  const int chunk = e->fluency_chunk, n_chunk = (N + chunk - 1) / chunk;
  {
    std::vector<int32_t> t2((size_t)5 * N + n_chunk + R);
    int32_t *ros = t2.data(), *cos_ = ros + N, *oidx = cos_ + N, *slen = oidx + N, *soff = slen + N, *lrow = soff + N + n_chunk;
    memcpy(ros, tab.data(), (size_t)N * 4);
    memcpy(cos_, tab.data() + (size_t)R * Lmax, (size_t)N * 4);
    for (int n = 0; n < N; ++n) {
      oidx[n] = ros[n] * Lmax + (cos_[n] - seed_len);
      slen[n] = len_of_row_host ? seed_len + len_of_row_host[ros[n]] + 1 : T;
    }
    for (int k = 0; k < n_chunk; ++k) {
      const int n0 = k * chunk, cn = std::min(chunk, N - n0);
      int32_t* off = soff + n0 + k;
      off[0] = 0;
      for (int i = 0; i < cn; ++i) off[i + 1] = off[i] + slen[n0 + i];
    }
    for (int r = 0; r < R; ++r) lrow[r] = len_of_row_host ? len_of_row_host[r] : Lmax;
    tab.swap(t2);
  }
  const int32_t *h_col = tab.data() + N, *h_slen = tab.data() + (size_t)3 * N, *h_soff = tab.data() + (size_t)4 * N;
  int *d_tab, *d_rows, *d_ids, *d_target, *d_gen, *d_rank, *flag; float *d_logp, *d_pll;
  E_CHECK(ensure(e, "s_nonfinite", 32, (void**)&flag));
  E_CHECK(ensure(e, "fl_tab", tab.size() * 4, (void**)&d_tab));
  E_CHECK(ensure(e, "fl_rows", n_ids * 4, (void**)&d_rows));
  E_CHECK(ensure(e, "fl_ids", (size_t)std::min(chunk, N) * T * 4, (void**)&d_ids));
  E_CHECK(ensure(e, "fl_target", (size_t)std::min(chunk, N) * 4, (void**)&d_target));
  E_CHECK(ensure(e, "fl_gen", (size_t)std::min(chunk, N) * 4, (void**)&d_gen));
  E_CHECK(ensure(e, "fl_logp", (size_t)R * Lmax * 4, (void**)&d_logp));
  E_CHECK(ensure(e, "fl_rank", (size_t)R * Lmax * 4, (void**)&d_rank));
  E_CHECK(ensure(e, "fl_pll", (size_t)R * 4, (void**)&d_pll));
  const int *d_ros = d_tab, *d_col = d_tab + N, *d_oidx = d_tab + (size_t)2 * N, *d_slen = d_tab + (size_t)3 * N,
            *d_soff = d_tab + (size_t)4 * N, *d_lrow = d_tab + (size_t)5 * N + n_chunk;
  // from here on BERT's buffers are this call's: whatever the call returns, no later n_mask = 0 step re-uses a forward, and
  // the host columns bert_forward is shown do not outlive the call
  struct EndReuse {
    czc_engine* e;
    ~EndReuse() { (void)hipStreamSynchronize(e->st); e->bert_pruned_idx = PRUNED_ROWS; e->bert_pruned_rows = nullptr; }
  } end_reuse{e};
  E_HIP(hipMemsetAsync(flag, 0, 32, e->st));
  E_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, e->st));
  E_HIP(hipMemcpyAsync(d_rows, rows, n_ids * 4, hipMemcpyDefault, e->st));
  E_HIP(hipMemsetAsync(d_logp, 0, (size_t)R * Lmax * 4, e->st));
  E_HIP(hipMemsetAsync(d_rank, 0xff, (size_t)R * Lmax * 4, e->st));  // -1
  const bool prune = e->bert_prune != 0;
  for (int k = 0; k < n_chunk; ++k) {
    const int n0 = k * chunk, cn = std::min(chunk, N - n0);
    { ProfScope ps(e, "rowops", 0);
      E_CHECK(launch_expand_mask_rows(d_rows, T, d_ros + n0, d_col + n0, cn, c.mask_id, d_ids, d_target, d_gen, e->st)); }
    Ragged rag{d_soff + n0 + k, d_slen + n0, h_soff[n0 + k + cn], 0};
    for (int i = 0; i < cn; ++i) rag.max_T = std::max(rag.max_T, h_slen[n0 + i]);
    const Ragged* rg = dense ? nullptr : &rag;
    E_CHECK(bert_forward(e, d_ids, cn, T, prune ? h_col[n0] : -1, prune ? d_gen : nullptr, h_col + n0, rg));
    float* logits;
    E_CHECK(mlm_head(e, cn, T, h_col[n0], &logits, d_gen, h_col + n0, rg));
    { ProfScope ps(e, "topk", 0);
      E_CHECK(launch_logprob_target(logits, cn, V, d_target, temperature, d_oidx + n0, d_logp, d_rank, flag, e->st)); }
  }
  if (out_pll) {
    ProfScope ps(e, "rowops", 0);
    E_CHECK(launch_pll_sum(d_logp, R, Lmax, d_lrow, d_pll, e->st));
    E_HIP(hipMemcpyAsync(out_pll, d_pll, (size_t)R * 4, hipMemcpyDefault, e->st));
  }
  if (out_logp) E_HIP(hipMemcpyAsync(out_logp, d_logp, (size_t)R * Lmax * 4, hipMemcpyDefault, e->st));
  if (out_rank) E_HIP(hipMemcpyAsync(out_rank, d_rank, (size_t)R * Lmax * 4, hipMemcpyDefault, e->st));
  E_HIP(hipMemcpyAsync(e->h_totals + HT_FLAGS, flag, 4, hipMemcpyDeviceToHost, e->st));
  E_HIP(hipStreamSynchronize(e->st));
  if (e->h_totals[HT_FLAGS]) return fail(e, CZC_ERR_OVERFLOW, "fluency_rows: non-finite log-probability (a non-finite BERT logit)%s");
  return CZC_OK;
}

int czc_set_control_callback(czc_engine* e, czc_control_fn fn, void* user) {
  if (!e) return CZC_ERR_ARG;
  e->ctl_fn = fn;
  e->ctl_user = fn ? user : nullptr;
  return CZC_OK;
}

int czc_set_option(czc_engine* e, const char* name, int value) {
  if (!e || !name) return CZC_ERR_ARG;
  if (!strcmp(name, "share_prefix")) { e->share_prefix = value ? 1 : 0; return CZC_OK; }
  if (!strcmp(name, "dedup")) { e->dedup = value ? 1 : 0; return CZC_OK; }
  if (!strcmp(name, "bert_prune")) { e->bert_prune = value ? 1 : 0; return CZC_OK; }
  if (!strcmp(name, "bert_fuse_splitk_ln")) { e->bert_fuse_splitk_ln = value ? 1 : 0; return CZC_OK; }
  if (!strcmp(name, "pack_branches")) { e->pack_branches = value ? 1 : 0; return CZC_OK; }
  if (!strcmp(name, "pool_last_layer")) { e->pool_last_layer = value ? 1 : 0; return CZC_OK; }
  if (!strcmp(name, "share_layer0")) { e->share_layer0 = value ? 1 : 0; return CZC_OK; }
  if (!strcmp(name, "pool_last_qkv")) { e->pool_last_qkv = value ? 1 : 0; return CZC_OK; }
  if (!strcmp(name, "fuse_ln")) { e->fuse_ln = value; return CZC_OK; }  // 0 off, 1 out-proj -> LN2, 2 also fc2 -> next LN1
  const auto fold_ready = [&]() -> int {  // an option that turns the folded form on after the weights were finalized without it
    if (e->finalized && wants_folded_ln(e) && (e->ctext.empty() || !e->ctext[0].qkv_wf))
      return fail(e, CZC_ERR_STATE, "option %s: this engine was finalized without the folded-LayerNorm operands (set it before czc_finalize_weights)", name);
    return CZC_OK;
  };
  if (!strcmp(name, "resid16")) { const int old = e->resid16; e->resid16 = value < 0 ? 0 : value; const int rc = fold_ready(); if (rc) e->resid16 = old; return rc; }
  if (!strcmp(name, "fold_ln")) { const int old = e->fold_ln; e->fold_ln = value ? 1 : 0; const int rc = fold_ready(); if (rc) e->fold_ln = old; return rc; }
  if (!strcmp(name, "refine_samples")) { e->refine_samples = value < 0 ? 0 : value; return CZC_OK; }
  if (!strcmp(name, "refine_samples_step")) { e->refine_samples_step = value < 0 ? 0 : value; return CZC_OK; }
  if (!strcmp(name, "refine_theta_x1000")) { e->refine_theta_x = (float)value / 1000.f; return CZC_OK; }
  if (!strcmp(name, "refine_theta_gen_x1000")) { e->refine_theta_gen = (float)value / 1000.f; return CZC_OK; }
  if (!strcmp(name, "refine_guard_x1e6")) { e->refine_guard_dev = (float)value * 1e-6f; return CZC_OK; }
  if (!strcmp(name, "refine_gate_x1e6")) { e->refine_gate_delta = value < 0 ? 0.f : (float)value * 1e-6f; return CZC_OK; }
  if (!strcmp(name, "refine_rows16")) { const int old = e->refine_rows16; e->refine_rows16 = value ? 1 : 0; const int rc = fold_ready(); if (rc) e->refine_rows16 = old; return rc; }
  if (!strcmp(name, "memo")) { e->memo = value ? 1 : 0; return CZC_OK; }
  if (!strcmp(name, "memo_rows")) { e->memo_rows = value ? 1 : 0; return CZC_OK; }
  if (!strcmp(name, "index_groups")) {
    if (value < 0 || value > 1024) return fail(e, CZC_ERR_ARG, "option %s: 0 (chosen by the launcher) or 1..1024", name);
    e->index_groups = value;
    return CZC_OK;
  }
  if (!strcmp(name, "fluency_chunk")) {
    if (value < 1 || value > 16384) return fail(e, CZC_ERR_ARG, "option %s: 1..16384", name);
    e->fluency_chunk = value;
    return CZC_OK;
  }
  if (!strcmp(name, "regions_chunk")) {
    if (value < 1 || value > CZC_MAX_REGIONS) return fail(e, CZC_ERR_ARG, "option %s: 1..1024", name);
    e->regions_chunk = value;
    return CZC_OK;
  }
  if (!strcmp(name, "refine_rows16_x1000")) { e->refine_rows16_factor = value < 1000 ? 1.f : (float)value / 1000.f; return CZC_OK; }
  return fail(e, CZC_ERR_ARG, "unknown option %s", name);
}

int czc_get_option(czc_engine* e, const char* name, int* value) {
  if (!e || !name || !value) return CZC_ERR_ARG;
  const bool r16 = e->refine && e->refine_rows16 && e->cfg.clip_hidden == 512;  // what czc_generate's screening pass runs on
  const float f16x = r16 ? e->refine_rows16_factor : 1.f;
  struct { const char* n; int v; } tab[] = {
      {"share_prefix", e->share_prefix}, {"bert_prune", e->bert_prune}, {"pack_branches", e->pack_branches},
      {"dedup", e->dedup}, {"pool_last_layer", e->pool_last_layer}, {"pool_last_qkv", e->pool_last_qkv}, {"share_layer0", e->share_layer0}, {"bert_fuse_splitk_ln", e->bert_fuse_splitk_ln}, {"fuse_ln", e->fuse_ln}, {"resid16", e->resid16}, {"fold_ln", e->fold_ln},
      {"refine_samples", e->refine_samples}, {"refine_samples_step", e->refine_samples_step}, {"refine_theta_x1000", (int)lrintf(e->refine_theta_x * 1000.f)},
      {"refine_theta_gen_x1000", (int)lrintf(e->refine_theta_gen * 1000.f)},
      {"refine_guard_x1e6", (int)lrintf(e->refine_guard_dev * 1e6f)}, {"refine_gate_x1e6", (int)lrintf(e->refine_gate_delta * 1e6f)},
      {"refine_rows16", e->refine_rows16}, {"memo", e->memo}, {"memo_rows", e->memo_rows}, {"index_groups", e->index_groups}, {"fluency_chunk", e->fluency_chunk}, {"regions_chunk", e->regions_chunk}, {"refine_rows16_x1000", (int)lrintf(e->refine_rows16_factor * 1000.f)},
      // read-only, derived: the trip point / gate bound in force inside czc_generate (x refine_rows16_factor on fp16 rows)
      {"refine_guard_generate_x1e6", (int)lrintf(e->refine_guard_dev * f16x * 1e6f)},
      {"refine_gate_generate_x1e6", (int)lrintf(e->refine_gate_delta * f16x * 1e6f)},
      {"has_folded_ln_weights", !e->ctext.empty() && e->ctext[0].qkv_wf ? 1 : 0},
  };
  for (auto& t : tab) if (!strcmp(name, t.n)) { *value = t.v; return CZC_OK; }
  return fail(e, CZC_ERR_ARG, "unknown option %s", name);
}

int czc_sync(czc_engine* e) {
  if (!e) return CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  E_HIP(hipStreamSynchronize(e->st));
  return CZC_OK;
}

int czc_profile_enable(czc_engine* e, int on) {
  if (!e) return CZC_ERR_ARG;
  e->prof = on < 0 ? 0 : (on > 2 ? 1 : on);
  return CZC_OK;
}

int czc_profile_reset(czc_engine* e) {
  if (!e) return CZC_ERR_ARG;
  (void)hipSetDevice(e->dev);  // the current device is per host thread (events are created on it)
  (void)hipStreamSynchronize(e->st);
  if (!e->prof_ref) (void)hipEventCreate(&e->prof_ref);
  if (e->prof_ref) (void)hipEventRecord(e->prof_ref, e->st);
  for (auto& kv : e->pk) { kv.second.used = 0; kv.second.flops = 0; kv.second.launches = 0; }
  e->stat_clip_rows = e->stat_clip_seqs = e->stat_bert_rows = e->stat_steps = 0;
  e->stat_refine_rows = e->stat_refine_seqs = 0;
  e->stat_dedup_seqs = 0;
  e->stat_gated = e->stat_gate_images = 0;
  e->stat_memo_hits = e->stat_memo_images = 0;
  e->stat_memo_row_hits = e->stat_memo_row_steps = 0;
  return CZC_OK;
}

int czc_profile_get(czc_engine* e, const char* kind, double* total_ms, int64_t* launches, double* flops) {
  if (!e || !kind) return CZC_ERR_ARG;
  E_HIP(hipSetDevice(e->dev));
  E_HIP(hipStreamSynchronize(e->st));
  double ms = 0;
  int64_t n = 0;
  double fl = 0;
  auto it = e->pk.find(kind);
  if (it != e->pk.end()) {
    ProfKind& k = it->second;
    for (size_t i = 0; i + 1 < k.used; i += 2) {
      float t = 0;
      if (hipEventElapsedTime(&t, k.ev[i], k.ev[i + 1]) == hipSuccess) ms += t;
    }
    n = k.launches;
    fl = k.flops;
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  if (flops) *flops = fl;
  return CZC_OK;
}

// Start / end (ms) of every launch of kernel class `kind` since czc_profile_reset(e), on the clock whose zero is
// czc_profile_reset(ref) (ref = e for one engine; the same ref for all engines that ran concurrently, so that the
// host can take the union of their intervals: the time the GPU spent on that class with the launches overlapping).
int czc_profile_intervals(czc_engine* e, czc_engine* ref, const char* kind, double* start_ms, double* end_ms, int cap,
                          int* n_out) {
  if (!e || !ref || !kind || !n_out || cap < 0 || (cap > 0 && (!start_ms || !end_ms))) return CZC_ERR_ARG;
  if (!ref->prof_ref) return fail(e, CZC_ERR_STATE, "czc_profile_intervals: czc_profile_reset the reference engine first%s");
  if (ref->dev != e->dev) return fail(e, CZC_ERR_ARG, "czc_profile_intervals: engines on different devices%s");
  E_HIP(hipSetDevice(e->dev));
  E_HIP(hipStreamSynchronize(e->st));
  E_HIP(hipStreamSynchronize(ref->st));
  int n = 0;
  auto it = e->pk.find(kind);
  if (it != e->pk.end()) {
    ProfKind& k = it->second;
    for (size_t i = 0; i + 1 < k.used; i += 2, ++n) {
      if (n >= cap) continue;
      float a = 0, b = 0;
      E_HIP(hipEventElapsedTime(&a, ref->prof_ref, k.ev[i]));
      E_HIP(hipEventElapsedTime(&b, ref->prof_ref, k.ev[i + 1]));
      start_ms[n] = a; end_ms[n] = b;
    }
  }
  *n_out = n;
  return CZC_OK;
}

int czc_stats(czc_engine* e, int64_t* clip_rows, int64_t* clip_seqs, int64_t* bert_rows, int64_t* steps) {
  if (!e) return CZC_ERR_ARG;
  if (clip_rows) *clip_rows = e->stat_clip_rows;
  if (clip_seqs) *clip_seqs = e->stat_clip_seqs;
  if (bert_rows) *bert_rows = e->stat_bert_rows;
  if (steps) *steps = e->stat_steps;
  return CZC_OK;
}

int czc_dedup_stats(czc_engine* e, int64_t* dedup_seqs, int64_t* clip_seqs) {
  if (!e) return CZC_ERR_ARG;
  if (dedup_seqs) *dedup_seqs = e->stat_dedup_seqs;
  if (clip_seqs) *clip_seqs = e->stat_clip_seqs;
  return CZC_OK;
}

int czc_refine_stats(czc_engine* e, int64_t* refine_seqs, int64_t* refine_rows) {
  if (!e) return CZC_ERR_ARG;
  if (refine_seqs) *refine_seqs = e->stat_refine_seqs;
  if (refine_rows) *refine_rows = e->stat_refine_rows;
  return CZC_OK;
}

int czc_refine_gate_stats(czc_engine* e, int64_t* gated, int64_t* image_steps) {
  if (!e) return CZC_ERR_ARG;
  if (gated) *gated = e->stat_gated;
  if (image_steps) *image_steps = e->stat_gate_images;
  return CZC_OK;
}

int czc_memo_stats(czc_engine* e, int64_t* hit_image_steps, int64_t* image_steps) {
  if (!e) return CZC_ERR_ARG;
  if (hit_image_steps) *hit_image_steps = e->stat_memo_hits;
  if (image_steps) *image_steps = e->stat_memo_images;
  return CZC_OK;
}

int czc_memo_rows_stats(czc_engine* e, int64_t* hit_row_steps, int64_t* row_steps) {
  if (!e) return CZC_ERR_ARG;
  if (hit_row_steps) *hit_row_steps = e->stat_memo_row_hits;
  if (row_steps) *row_steps = e->stat_memo_row_steps;
  return CZC_OK;
}

int czc_refine_guard(czc_engine* e, int reset, float* max_dev, int64_t* tripped) {
  if (!e) return CZC_ERR_ARG;
  if (max_dev) *max_dev = e->guard_max_dev;
  if (tripped) *tripped = e->guard_trips;
  if (reset) { e->guard_max_dev = 0.f; e->guard_trips = 0; }
  return CZC_OK;
}

// czc_test_text_tower (api_test.hip): the engine's text tower on host-given CLIP id rows of B images x K candidates, through the
// step's own plan (shared prefix and de-duplication as the engine's options say) -> features [B*K, proj]; *n_dup = candidates that
// ride on an identical one
static int test_text_tower(void* engine, const int32_t* clip_ids, const int32_t* clip_len, int B, int K, float* out, int32_t* n_dup) {
  czc_engine* e = (czc_engine*)engine;
  if (!e || !clip_ids || !clip_len || B <= 0 || K <= 0 || K > CZC_MAX_TOPK || !out) return CZC_ERR_ARG;
  TowerPlan tp;
  E_CHECK(text_features(e, clip_ids, clip_len, B, K, e->share_prefix, false, out, &tp));  // the engine's own rows
  if (n_dup) *n_dup = tp.n_dup;
  return CZC_OK;
}

const void* czc_internal_hooks(int abi) {
  static const Hooks h = {
      []() -> char* { return czc::g_err; },
      &launch_gemm, &launch_gemm_rowln, &launch_layernorm, &launch_convert, &launch_act_to_f32, &launch_attention,
      &launch_attention_shared, &launch_attention_shared_split,
      &launch_softmax_mask_topk, &launch_bridge_precompute, &launch_bridge, &launch_l2_normalize, &launch_combine,
      &launch_layernorm_x16, &launch_ln_finalize, &launch_fold_ln, &gemm_wreg_stats_in_kernel,
      &g_use_gemm256, &g_use_skinny, &g_use_splitk, &g_gemm_deep, &g_gemm_small_tiles, &g_use_wreg, &g_use_gemm256s,
      &g_rowln_min_m, &g_wreg_min_m, &g_gemm256_min_m, &g_use_mfma_attention, &g_use_attention_image, &g_wreg_resid_min_m,
      &g_wreg_stats_in_kernel, &g_gemm256s_min_m,
      &launch_scan, &launch_prefix_plan, &launch_prefix_finish, &launch_refine_select, &launch_refine_select_rows,
      &launch_refine_select_draw, &launch_refine_plan, &launch_refine_finish, &launch_refine_cosine,
      &launch_attention_image_pooled, &launch_attention_shared_mapped, &launch_layer0_count, &launch_layer0_map,
      &test_text_tower,
      &launch_layernorm_splitk, &launch_bert_embed, &launch_bert_embed_ragged, &launch_clip_embed, &launch_im2col, &launch_vision_assemble,
      &launch_gather_rows_f32, &launch_gather_rows_bytes, &launch_gather_rows_w32, &launch_mask_positions, &launch_mask_positions_rows,
      &launch_tie_rows, &launch_memo_check, &launch_memo_gather, &launch_memo_scatter, &launch_memo_fill, &launch_memo_rows_check,
      &launch_memo_rows_gather, &launch_memo_rows_scatter, &launch_memo_rows_fill,
      &fluency_expand_tables, &launch_expand_mask_rows, &launch_logprob_target,
      &launch_bridge_rows, &launch_bridge_rows_hp, &launch_softmax_mask_topk_rows, &launch_softmax_mask_topk_rows_hp,
      &launch_softmax_mask_topk_rows_vocab,
      []() -> int { return czc::g_gemm_family; },
      &launch_gather_row_hyper, &launch_gather_row_draw};
  return abi == HOOKS_ABI ? &h : nullptr;
}

}  // extern "C"
