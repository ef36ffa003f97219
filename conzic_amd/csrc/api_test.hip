// Kernel-level parity hooks of include/conzic_hip_test.h (czc_test_*): run ONE kernel on host data.
// Used only by tests/ (-m gpu) to compare each HIP kernel with the CPU oracle, and by tools/ for kernel A/B timing.
// Built into libconzic_hip_test.so, which links against the product library's C ABI only (czc_internal_hooks).
#include <vector>
#include <cstring>
#include <algorithm>
#include <cstdlib>

#include "../../include/conzic_hip_test.h"
#include "kernels.h"
#include "bridge_hash.h"

#include "../../include/conzic_hip.h"

using namespace czc;

// everything this file needs from inside libconzic_hip.so comes through its one internal door (the product library
// exports its C ABI and nothing else): launchers, the calling thread's error buffer, the kernel-family switches
static const Hooks& HK() {
  static const Hooks* h = (const Hooks*)czc_internal_hooks(HOOKS_ABI);
  if (!h) { fprintf(stderr, "libconzic_hip_test.so: libconzic_hip.so was built from another tree (hooks ABI)\n"); abort(); }
  return *h;
}
#define launch_gemm HK().gemm
#define launch_gemm_rowln HK().gemm_rowln
#define launch_layernorm HK().layernorm
#define launch_convert HK().convert
#define launch_act_to_f32 HK().act_to_f32
#define launch_attention HK().attention
#define launch_attention_shared HK().attention_shared
#define launch_attention_shared_split HK().attention_shared_split
#define launch_softmax_mask_topk HK().softmax_mask_topk
#define launch_bridge_precompute HK().bridge_precompute
#define launch_bridge HK().bridge
#define launch_l2_normalize HK().l2_normalize
#define launch_combine HK().combine
#define launch_layernorm_x16 HK().layernorm_x16
#define launch_ln_finalize HK().ln_finalize
#define launch_fold_ln HK().fold_ln
#define gemm_wreg_stats_in_kernel HK().wreg_stats_ok
#define launch_scan HK().scan
#define launch_prefix_plan HK().prefix_plan
#define launch_prefix_finish HK().prefix_finish
#define launch_refine_select HK().refine_select
#define launch_refine_select_rows HK().refine_select_rows
#define launch_refine_select_draw HK().refine_select_draw
#define launch_refine_plan HK().refine_plan
#define launch_refine_finish HK().refine_finish
#define launch_refine_cosine HK().refine_cosine
#define launch_gather_row_hyper HK().gather_row_hyper
#define launch_gather_row_draw HK().gather_row_draw
#define g_use_gemm256 (*HK().use_gemm256)
#define g_use_skinny (*HK().use_skinny)
#define g_use_splitk (*HK().use_splitk)
#define g_gemm_deep (*HK().gemm_deep)
#define g_gemm_small_tiles (*HK().gemm_small_tiles)
#define g_use_wreg (*HK().use_wreg)
#define g_use_gemm256s (*HK().use_gemm256s)
#define g_rowln_min_m (*HK().rowln_min_m)
#define g_wreg_min_m (*HK().wreg_min_m)
#define g_gemm256_min_m (*HK().gemm256_min_m)
#define g_gemm256s_min_m (*HK().gemm256s_min_m)
#define g_use_mfma_attention (*HK().use_mfma_attention)
#define g_use_attention_image (*HK().use_attention_image)
#define g_wreg_resid_min_m (*HK().wreg_resid_min_m)
#define g_wreg_stats_in_kernel (*HK().wreg_stats_in_kernel)
#define TEST_ERR (HK().err_buf())

static int g_bench_pad = 0;
static int g_bridge_no_table = 0;  // czc_test_bridge, czc_test_bridge_cand: 1 = every chunk through the merge loop (option "bridge_no_table")  // czc_bench_gemm: extra elements per row of A and W (row pitch vs L2 channel experiments)

namespace {

struct DevPool {
  std::vector<void*> ptrs;
  ~DevPool() { for (void* p : ptrs) (void)hipFree(p); }
  void* alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return p;
  }
  void* up(const void* src, size_t bytes) {
    void* p = alloc(bytes);
    if (p && src && hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
  }
};

#define T_HIP(expr)                                                                                   \
  do {                                                                                                \
    hipError_t _h = (expr);                                                                           \
    if (_h != hipSuccess) {                                                                           \
      snprintf(TEST_ERR, 512, "%s:%d %s -> %s", __FILE__, __LINE__, #expr,           \
               hipGetErrorString(_h));                                                                \
      return CZC_ERR_HIP;                                                                             \
    }                                                                                                 \
  } while (0)
#define T_CHECK(expr) do { int _r = (expr); if (_r) return _r; } while (0)
#define T_PTR(p) do { if (!(p)) { snprintf(TEST_ERR, 512, "device allocation/copy failed"); return CZC_ERR_HIP; } } while (0)

// fp32 host -> device buffer in precision `prec`
void* up_act(DevPool& pool, int prec, const float* src, size_t n) {
  float* f = (float*)pool.up(src, n * 4);
  if (!f) return nullptr;
  if (prec == PREC_F32) return f;
  void* a = pool.alloc(n * prec_bytes(prec));
  if (!a) return nullptr;
  if (launch_convert(prec, f, a, (long)n, nullptr)) return nullptr;
  return a;
}

int down_act(DevPool& pool, int prec, const void* src, size_t n, float* host) {
  const float* f = (const float*)src;
  if (prec != PREC_F32) {
    float* t = (float*)pool.alloc(n * 4);
    T_PTR(t);
    T_CHECK(launch_act_to_f32(prec, src, t, (long)n, nullptr));
    f = t;
  }
  T_HIP(hipMemcpy(host, f, n * 4, hipMemcpyDeviceToHost));
  return 0;
}

// An output buffer of n 4-byte words inside a larger allocation (the selection / plan hooks): CZC_TEST_GUARD words in front of
// it and behind it, everything pre-filled with bytes 0x5a, and all n + 2 * CZC_TEST_GUARD words go back to the caller -- a stray
// store shows in the result instead of leaving the buffer, and a word a kernel does not write reads back as the pattern.
struct Guarded {
  unsigned char* base = nullptr;
  size_t n = 0;
  template <typename T> T* p() const { return (T*)(base + (size_t)CZC_TEST_GUARD * 4); }
  int make(DevPool& pool, size_t words) {
    n = words;
    base = (unsigned char*)pool.alloc((n + 2 * CZC_TEST_GUARD) * 4); T_PTR(base);
    T_HIP(hipMemset(base, 0x5a, (n + 2 * CZC_TEST_GUARD) * 4));
    return 0;
  }
  int zero(size_t words) const {  // the engine's own memset of (part of) the buffer
    T_HIP(hipMemset(base + (size_t)CZC_TEST_GUARD * 4, 0, words * 4));
    return 0;
  }
  int fill(const void* src) const {
    T_HIP(hipMemcpy(base + (size_t)CZC_TEST_GUARD * 4, src, n * 4, hipMemcpyHostToDevice));
    return 0;
  }
  int down(void* host) const {
    T_HIP(hipMemcpy(host, base, (n + 2 * CZC_TEST_GUARD) * 4, hipMemcpyDeviceToHost));
    return 0;
  }
};

// The bridge tables on the device as the engine holds them (czc_set_bridge): the arrays uploaded, the merge list hashed and --
// unless the option "bridge_no_table" is set -- the per-token CLIP ids tabulated by launch_bridge_precompute.  Shared by
// czc_test_bridge and czc_test_bridge_cand.
int bridge_tables_dev(DevPool& pool, const czc_bridge_tables* t, BridgeDev& bd) {
  const size_t nbytes = t->piece_off[t->bert_vocab];
  bd.bert_vocab = t->bert_vocab;
  bd.piece_off = (const uint32_t*)pool.up(t->piece_off, (size_t)(t->bert_vocab + 1) * 4); T_PTR(bd.piece_off);
  bd.piece_bytes = (const uint8_t*)pool.up(t->piece_bytes, nbytes ? nbytes : 1); T_PTR(bd.piece_bytes);
  bd.piece_class = (const uint8_t*)pool.up(t->piece_class, nbytes ? nbytes : 1); T_PTR(bd.piece_class);
  bd.piece_flags = (const uint8_t*)pool.up(t->piece_flags, (size_t)t->bert_vocab); T_PTR(bd.piece_flags);
  bd.byte_sym = (const int*)pool.up(t->byte_sym, 256 * 4); T_PTR(bd.byte_sym);
  bd.byte_sym_eow = (const int*)pool.up(t->byte_sym_eow, 256 * 4); T_PTR(bd.byte_sym_eow);
  size_t cap = 1024;
  while (cap < (size_t)t->n_merges * 2 + 2) cap <<= 1;
  std::vector<unsigned long long> keys(cap, ~0ull), vals(cap, 0ull);
  for (int r = 0; r < t->n_merges; ++r) {
    const unsigned long long key = ((unsigned long long)(unsigned)t->merge_left[r] << 32) | (unsigned)t->merge_right[r];
    unsigned h = bridge_hash(key) & (unsigned)(cap - 1);
    bool dup = false;
    while (keys[h] != ~0ull) {
      if (keys[h] == key) { dup = true; break; }
      h = (h + 1) & (unsigned)(cap - 1);
    }
    if (dup) continue;
    keys[h] = key;
    vals[h] = ((unsigned long long)(unsigned)r << 32) | (unsigned)t->merge_out[r];
  }
  bd.hkeys = (const unsigned long long*)pool.up(keys.data(), cap * 8); T_PTR(bd.hkeys);
  bd.hvals = (const unsigned long long*)pool.up(vals.data(), cap * 8); T_PTR(bd.hvals);
  bd.hmask = (unsigned)(cap - 1);
  bd.bos_id = t->bos_id;
  bd.eos_id = t->eos_id;
  if (!g_bridge_no_table) {  // the product's fast path: per-token ids tabulated on the device
    int* tok_ids = (int*)pool.alloc((size_t)t->bert_vocab * BR_TOKMAX * 4); T_PTR(tok_ids);
    uint8_t* tok_len = (uint8_t*)pool.alloc((size_t)t->bert_vocab); T_PTR(tok_len);
    T_CHECK(launch_bridge_precompute(bd, tok_ids, tok_len, nullptr));
    T_HIP(hipDeviceSynchronize());
    bd.tok_bpe = tok_ids; bd.tok_bpe_len = tok_len;
  }
  return 0;
}

}  // namespace

extern "C" {

int czc_test_gemm(int precision, int M, int N, int K, const float* A, const float* W, const float* bias,
                  const float* resid, int act, float* C) {
  DevPool pool;
  void* dA = up_act(pool, precision, A, (size_t)M * K); T_PTR(dA);
  void* dW = up_act(pool, precision, W, (size_t)N * K); T_PTR(dW);
  float* dB = bias ? (float*)pool.up(bias, (size_t)N * 4) : nullptr;
  float* dR = resid ? (float*)pool.up(resid, (size_t)M * N * 4) : nullptr;
  const bool typed_out = (act & 0x100) != 0;  // store through the activation-typed epilogue (bf16 / split / f32)
  act &= 0xff;
  GemmArgs g;
  g.A = dA; g.lda = K; g.W = dW; g.ldw = K; g.bias = dB; g.resid = dR; g.ldr = N;
  g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = act;
  if (typed_out) {
    void* dO = pool.alloc((size_t)M * N * prec_bytes(precision)); T_PTR(dO);
    g.out_act = dO; g.out_f32 = nullptr;
    T_CHECK(launch_gemm(precision, g, nullptr));
    T_HIP(hipDeviceSynchronize());
    return down_act(pool, precision, dO, (size_t)M * N, C);
  }
  float* dC = (float*)pool.alloc((size_t)M * N * 4); T_PTR(dC);
  g.out_act = nullptr; g.out_f32 = dC;
  T_CHECK(launch_gemm(precision, g, nullptr));
  T_HIP(hipDeviceSynchronize());
  T_HIP(hipMemcpy(C, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost));
  return 0;
}

// The residual-add layers on a 2-byte residual stream (GemmArgs::x16): x_out = fp16(fp16(resid) + A.W^T + bias), in place on the
// fp16 rows as the engine runs it; which kernel serves it follows the shape and the czc_test_set_option switches (weight-stationary
// residual kernel at K = 512 / N % 256 == 0, ping-pong ring kernel from gemm256_min_m rows, tiled kernel otherwise).
int czc_test_gemm_x16(int precision, int M, int N, int K, const float* A, const float* W, const float* bias, const float* resid,
                      float* x_out, float* part_out) {
  if (precision != PREC_BF16 && precision != PREC_F16) { snprintf(TEST_ERR, 512, "gemm_x16: bf16 / fp16 operands only"); return CZC_ERR_ARG; }
  DevPool pool;
  void* dA = up_act(pool, precision, A, (size_t)M * K); T_PTR(dA);
  void* dW = up_act(pool, precision, W, (size_t)N * K); T_PTR(dW);
  float* dB = bias ? (float*)pool.up(bias, (size_t)N * 4) : nullptr;
  void* dx = up_act(pool, PREC_F16, resid, (size_t)M * N); T_PTR(dx);
  GemmArgs g;
  g.A = dA; g.lda = K; g.W = dW; g.ldw = K; g.bias = dB; g.resid = (const float*)dx; g.ldr = N; g.out_act = nullptr;
  g.out_f32 = (float*)dx; g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = ACT_NONE; g.x16 = 1;
  float* dpart = nullptr;
  if (part_out) {  // LayerNorm partials [N / 32][M] float2 of the rows written
    dpart = (float*)pool.alloc((size_t)(N / 32) * M * 8); T_PTR(dpart);
    T_HIP(hipMemset(dpart, 0xff, (size_t)(N / 32) * M * 8));
    g.row_part = dpart; g.part_ld = M;
  }
  T_CHECK(launch_gemm(precision, g, nullptr));
  T_HIP(hipDeviceSynchronize());
  if (part_out) T_HIP(hipMemcpy(part_out, dpart, (size_t)(N / 32) * M * 8, hipMemcpyDeviceToHost));
  return down_act(pool, PREC_F16, dx, (size_t)M * N, x_out);
}

// LayerNorm folded into the weight-stationary K = 512 GEMM: out[M,N] = act( LN(fp16(x); gamma, beta, eps) . W^T + bias ) in the
// operand type of `precision`, computed as rstd * (x . W"^T) + b' from x itself: centred weights prepared by fold_ln_kernel
// (rowsum_out, optional [N]: what is left of each stored row's sum), statistics by ln_finalize_kernel from the partials `part`
// [16][M] float2 the caller supplies (a producer GEMM would have written them).
int czc_test_ln_fold_gemm(int precision, int M, int N, const float* x, const float* W, const float* gamma, const float* beta,
                          const float* bias, const float* part, float eps, int act, float* out, float* rowsum_out) {
  const int K = 512;
  if (precision != PREC_BF16 && precision != PREC_F16) { snprintf(TEST_ERR, 512, "ln_fold_gemm: bf16 / fp16 engines only"); return CZC_ERR_ARG; }
  DevPool pool;
  void* dx = up_act(pool, PREC_F16, x, (size_t)M * K); T_PTR(dx);
  float* dW = (float*)pool.up(W, (size_t)N * K * 4); T_PTR(dW);
  float* dg = (float*)pool.up(gamma, K * 4); T_PTR(dg);
  float* dbt = (float*)pool.up(beta, K * 4); T_PTR(dbt);
  float* db = bias ? (float*)pool.up(bias, (size_t)N * 4) : nullptr;
  float* dpart = (float*)pool.up(part, (size_t)16 * M * 8); T_PTR(dpart);
  float* dstat = (float*)pool.alloc((size_t)M * 8 + 256); T_PTR(dstat);
  void* dWf = pool.alloc((size_t)N * K * 2); T_PTR(dWf);
  float* dcs = (float*)pool.alloc((size_t)N * 4); T_PTR(dcs);
  float* dbf = (float*)pool.alloc((size_t)N * 4); T_PTR(dbf);
  void* dout = pool.alloc((size_t)M * N * 2); T_PTR(dout);
  const bool in_kernel = gemm_wreg_stats_in_kernel(M, N);  // small launches: the consumer sums the partials itself (option wreg_stats_in_kernel)
  if (!in_kernel) T_CHECK(launch_ln_finalize(dpart, M, 16, M, eps, dstat, nullptr));
  T_CHECK(launch_fold_ln(dW, dg, dbt, db, N, K, dWf, dcs, dbf, nullptr));
  GemmArgs g;
  g.A = dx; g.lda = K; g.W = dWf; g.ldw = K; g.bias = dbf; g.resid = nullptr; g.ldr = 0; g.out_act = dout; g.out_f32 = nullptr; g.ldc = N;
  g.M = M; g.N = N; g.K = K; g.act = act;
  g.ln_stat = dstat;
  if (in_kernel) { g.ln_part = dpart; g.ln_part_ld = M; g.ln_eps = eps; }
  T_CHECK(launch_gemm(precision, g, nullptr));
  T_HIP(hipDeviceSynchronize());
  if (rowsum_out) T_HIP(hipMemcpy(rowsum_out, dcs, (size_t)N * 4, hipMemcpyDeviceToHost));
  return down_act(pool, precision, dout, (size_t)M * N, out);
}

// LayerNorm of fp16 rows (512 wide) into the operand type: y = LN(fp16(x))
int czc_test_layernorm_x16(int precision, int M, const float* x, const float* gamma, const float* beta, float eps, float* y) {
  DevPool pool;
  void* dx = up_act(pool, PREC_F16, x, (size_t)M * 512); T_PTR(dx);
  float* dg = (float*)pool.up(gamma, 512 * 4); T_PTR(dg);
  float* db = (float*)pool.up(beta, 512 * 4); T_PTR(db);
  void* dy = pool.alloc((size_t)M * 512 * 2); T_PTR(dy);
  T_CHECK(launch_layernorm_x16(precision, dx, nullptr, dg, db, eps, M, 512, dy, nullptr));
  T_HIP(hipDeviceSynchronize());
  return down_act(pool, precision, dy, (size_t)M * 512, y);
}

// Microbenchmark of the GEMM kernels on device-resident random data (tools/bench_gemm.py).
// out_mode 0: bf16/act output (+bias, act); 1: fp32 output with in-place fp32 residual (+bias).
int czc_bench_gemm(int precision, int M, int N, int K, int act, int out_mode, int iters, int use256, double* ms_out) {
  DevPool pool;
  const size_t es = prec_bytes(precision);
  std::vector<float> ha((size_t)1 << 20), hw((size_t)N * K), hb(N);
  unsigned s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 32768.0f - 1.0f; };
  for (auto& v : ha) v = rnd();
  for (auto& v : hw) v = rnd() * 0.05f;
  for (auto& v : hb) v = rnd();
  const int pad = g_bench_pad;
  const size_t Kp = (size_t)K + pad;
  void* dA = pool.alloc((size_t)M * Kp * es); T_PTR(dA);
  float* tmp = (float*)pool.up(ha.data(), ha.size() * 4); T_PTR(tmp);
  for (size_t off = 0; off < (size_t)M * Kp; off += ha.size()) {
    const size_t n = std::min(ha.size(), (size_t)M * Kp - off);
    T_CHECK(launch_convert(precision, tmp, (char*)dA + off * es, (long)n, nullptr));
  }
  void* dW = nullptr;
  if (pad) {
    std::vector<float> hwp((size_t)N * Kp);
    for (auto& v : hwp) v = rnd() * 0.05f;
    dW = up_act(pool, precision, hwp.data(), hwp.size());
  } else {
    dW = up_act(pool, precision, hw.data(), hw.size());
  }
  T_PTR(dW);
  float* dB = (float*)pool.up(hb.data(), hb.size() * 4); T_PTR(dB);
  void* dOa = nullptr; float* dOf = nullptr;
  // out_mode: 0 activation-typed output; 1 fp32 output + fp32 residual (in place); 4 full-row kernel with the LayerNorm in
  // its epilogue; 5 the GEMM + LayerNorm pair it replaces
  if (out_mode == 0) { dOa = pool.alloc((size_t)M * N * es); T_PTR(dOa); }
  else { dOf = (float*)pool.alloc((size_t)M * N * 4); T_PTR(dOf); T_HIP(hipMemset(dOf, 0, (size_t)M * N * 4)); }
  GemmArgs g;
  g.A = dA; g.lda = (int)Kp; g.W = dW; g.ldw = (int)Kp; g.bias = dB; g.resid = dOf; g.ldr = N; g.out_act = dOa; g.out_f32 = dOf;
  g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = act;
  if (out_mode == 6) { g.x16 = 1; }  // 6: fp16 residual stream in place (the fp32 buffer doubles as M x N fp16 rows)
  if (out_mode == 7) {  // 7: folded-LayerNorm consumer (K = 512): the operands' bytes read as fp16, unit statistics
    float* dstat = (float*)pool.alloc((size_t)M * 8 + 256); T_PTR(dstat);
    std::vector<float> hs((size_t)M * 2);
    for (size_t i = 0; i < hs.size(); i += 2) { hs[i] = 0.1f; hs[i + 1] = 1.0f; }
    T_HIP(hipMemcpy(dstat, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
    g.ln_stat = dstat;
    g.out_act = pool.alloc((size_t)M * N * es); T_PTR(g.out_act);
    g.out_f32 = nullptr; g.resid = nullptr;
  }
  if (out_mode == 4 || out_mode == 5) {  // 4: full-row kernel with the LayerNorm in its epilogue; 5: the pair it replaces
    g.out_act = pool.alloc((size_t)M * N * 2); T_PTR(g.out_act);
    g.ln_gamma = dB; g.ln_beta = dB; g.ln_eps = 1e-5f; g.f16 = precision == PREC_F16;
  }
  const int saved = g_use_gemm256, saved_wreg = g_use_wreg;
  // use256: 0 128x128 kernel; 1 default choice of the ring kernels; 3 loader-wave ring kernel; 7 ping-pong ring kernel;
  // 6 weight-stationary kernel where eligible (else the default ring kernel)
  g_use_gemm256 = use256 == 7 ? 5 : use256 == 6 ? 1 : use256;
  g_use_wreg = use256 == 6 ? 1 : 0;
  hipEvent_t e0, e1;
  T_HIP(hipEventCreate(&e0)); T_HIP(hipEventCreate(&e1));
  auto run = [&]() -> int {
    if (out_mode == 4) return launch_gemm_rowln(g, nullptr);
    if (out_mode == 5) {
      GemmArgs p = g;
      p.out_act = nullptr; p.ln_gamma = p.ln_beta = nullptr;
      T_CHECK(launch_gemm(precision, p, nullptr));
      return launch_layernorm(precision, g.out_f32, nullptr, g.ln_gamma, g.ln_beta, g.ln_eps, M, N, g.out_act, nullptr, nullptr);
    }
    return launch_gemm(precision, g, nullptr);
  };
  for (int i = 0; i < 2; ++i) T_CHECK(run());
  T_HIP(hipDeviceSynchronize());
  T_HIP(hipEventRecord(e0, nullptr));
  for (int i = 0; i < iters; ++i) T_CHECK(run());
  T_HIP(hipEventRecord(e1, nullptr));
  T_HIP(hipEventSynchronize(e1));
  float ms = 0;
  T_HIP(hipEventElapsedTime(&ms, e0, e1));
  g_use_gemm256 = saved;
  g_use_wreg = saved_wreg;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  *ms_out = ms / iters;
  return 0;
}

// Full-row GEMM with the LayerNorm in its epilogue (gemm_rowln_kernel; bf16 or fp16 operands, N = 512):
//   x_out = resid + A[M,K].W[512,K]^T + bias;  y_out = LayerNorm(x_out; gamma, beta, eps) rounded to the operand type
int czc_test_gemm_rowln(int precision, int M, int K, const float* A, const float* W, const float* bias, const float* resid,
                        const float* gamma, const float* beta, float eps, float* x_out, float* y_out) {
  const int H = 512;
  if (precision != PREC_BF16 && precision != PREC_F16) { snprintf(TEST_ERR, 512, "gemm_rowln: bf16 / fp16 only"); return CZC_ERR_ARG; }
  DevPool pool;
  void* dA = up_act(pool, precision, A, (size_t)M * K); T_PTR(dA);
  void* dW = up_act(pool, precision, W, (size_t)H * K); T_PTR(dW);
  float* dB = bias ? (float*)pool.up(bias, (size_t)H * 4) : nullptr;
  float* dx = (float*)pool.up(resid, (size_t)M * H * 4); T_PTR(dx);
  float* dg = (float*)pool.up(gamma, (size_t)H * 4); T_PTR(dg);
  float* dbt = (float*)pool.up(beta, (size_t)H * 4); T_PTR(dbt);
  void* dy = pool.alloc((size_t)M * H * 2); T_PTR(dy);
  GemmArgs g;
  g.A = dA; g.lda = K; g.W = dW; g.ldw = K; g.bias = dB; g.resid = dx; g.ldr = H; g.out_act = dy; g.out_f32 = dx;
  g.ldc = H; g.M = M; g.N = H; g.K = K; g.act = ACT_NONE; g.f16 = precision == PREC_F16;
  g.ln_gamma = dg; g.ln_beta = dbt; g.ln_eps = eps;
  const int saved = g_rowln_min_m;
  g_rowln_min_m = 1;
  const int rc = launch_gemm_rowln(g, nullptr);
  g_rowln_min_m = saved;
  T_CHECK(rc);
  T_HIP(hipDeviceSynchronize());
  T_HIP(hipMemcpy(x_out, dx, (size_t)M * H * 4, hipMemcpyDeviceToHost));
  return down_act(pool, precision, dy, (size_t)M * H, y_out);
}

int czc_test_set_option(const char* name, int value) {
  if (!strcmp(name, "gemm256")) { g_use_gemm256 = value; return 0; }
  if (!strcmp(name, "skinny")) { g_use_skinny = value; return 0; }
  if (!strcmp(name, "splitk")) { g_use_splitk = value; return 0; }
  if (!strcmp(name, "gemm_deep")) { g_gemm_deep = value; return 0; }
  if (!strcmp(name, "gemm_small_tiles")) { g_gemm_small_tiles = value; return 0; }
  if (!strcmp(name, "bridge_no_table")) { g_bridge_no_table = value; return 0; }
  if (!strcmp(name, "wreg")) { g_use_wreg = value; return 0; }
  if (!strcmp(name, "gemm256s")) { g_use_gemm256s = value; return 0; }
  if (!strcmp(name, "bench_pad")) { g_bench_pad = value; return 0; }
  if (!strcmp(name, "rowln_min_m")) { g_rowln_min_m = value; return 0; }
  if (!strcmp(name, "wreg_min_m")) { g_wreg_min_m = value; return 0; }
  if (!strcmp(name, "gemm256_min_m")) { g_gemm256_min_m = value; return 0; }
  if (!strcmp(name, "gemm256s_min_m")) { g_gemm256s_min_m = value; return 0; }
  if (!strcmp(name, "mfma_attention")) { g_use_mfma_attention = value; return 0; }
  if (!strcmp(name, "attention_image")) { g_use_attention_image = value; return 0; }
  if (!strcmp(name, "wreg_resid_min_m")) { g_wreg_resid_min_m = value; return 0; }
  if (!strcmp(name, "wreg_stats_in_kernel")) { g_wreg_stats_in_kernel = value; return 0; }
  snprintf(TEST_ERR, 512, "unknown option %s", name);
  return CZC_ERR_ARG;
}

int czc_test_layernorm(int precision, int M, int H, const float* x, const float* gamma, const float* beta, float eps,
                       float* y) {
  DevPool pool;
  float* dx = (float*)pool.up(x, (size_t)M * H * 4); T_PTR(dx);
  float* dg = (float*)pool.up(gamma, (size_t)H * 4); T_PTR(dg);
  float* db = (float*)pool.up(beta, (size_t)H * 4); T_PTR(db);
  void* dy = pool.alloc((size_t)M * H * 4); T_PTR(dy);
  T_CHECK(launch_layernorm(precision, dx, nullptr, dg, db, eps, M, H, dy, nullptr, nullptr));
  T_HIP(hipDeviceSynchronize());
  T_CHECK(down_act(pool, precision, dy, (size_t)M * H, y));
  return 0;
}

int czc_test_attention(int precision, int n_seq, const int32_t* seq_len, int heads, int causal, float scale,
                       const float* qkv, float* out) {
  DevPool pool;
  std::vector<int> off(n_seq + 1, 0);
  int mx = 0;
  for (int i = 0; i < n_seq; ++i) { off[i + 1] = off[i] + seq_len[i]; mx = seq_len[i] > mx ? seq_len[i] : mx; }
  const size_t M = off[n_seq];
  const int Hd = heads * 64;
  void* dq = up_act(pool, precision, qkv, M * 3 * Hd); T_PTR(dq);
  int* doff = (int*)pool.up(off.data(), (n_seq + 1) * 4); T_PTR(doff);
  int* dlen = (int*)pool.up(seq_len, n_seq * 4); T_PTR(dlen);
  void* dout = pool.alloc(M * Hd * 4); T_PTR(dout);
  SegTable tab{nullptr, nullptr, doff, dlen, n_seq, 0};
  T_CHECK(launch_attention(precision, dq, tab, mx, heads, causal, scale, dout, nullptr));
  T_HIP(hipDeviceSynchronize());
  T_CHECK(down_act(pool, precision, dout, M * Hd, out));
  return 0;
}

// One attention launch on a shared-prefix plan laid out as the engine lays it out (kernels.h: launch_prefix_plan /
// launch_prefix_finish): segments 0..B-1 are the trunks (pre_len 0), segment B + b*K + k is branch (b,k) with pre_off =
// own_off[b], pre_len = trunk_len[b]; rows back to back, own_off = exclusive scan.  kernel 0: launch_attention (the generic
// per-segment kernels in their prefix form); 1: launch_attention_shared[_split] with the per-image kernel off; 2: the same with
// the per-image kernel forced.  qkv and out carry CZC_TEST_PLAN_GUARD rows in front of and behind the plan rows inside their
// own allocations: NaN patterns of the operand type in qkv, bytes 0x5a in out, so that a stray read or write shows in the
// result instead of leaving the buffer.  `out` receives all rows + 2 * guard rows.
int czc_test_attention_plan(int precision, int kernel, int B, int K, int heads, float scale, const int32_t* trunk_len,
                            const int32_t* own_len, int pass_img_max, const float* qkv, float* out) {
  const bool half = precision == PREC_BF16 || precision == PREC_F16;
  if (!(half || precision == PREC_F32 || precision == PREC_F16X3) || kernel < 0 || kernel > 2 || (kernel && precision == PREC_F32) ||
      (kernel == 2 && !half) || B < 1 || K < 1 || heads < 1 || (long)B * K > (1 << 22)) {
    snprintf(TEST_ERR, 512, "attention_plan: no kernel %d for precision %d (B %d K %d heads %d)", kernel, precision, B, K, heads);
    return CZC_ERR_ARG;
  }
  const int n_seg = B + B * K, GR = CZC_TEST_PLAN_GUARD;
  std::vector<int> len(n_seg), off(n_seg + 1, 0), poff(n_seg, 0), plen(n_seg, 0), imax(B, 0);
  int max_own = 0, max_keys = 0;
  for (int b = 0; b < B; ++b) len[b] = trunk_len[b];
  for (int i = 0; i < B * K; ++i) len[B + i] = own_len[i];
  for (int s = 0; s < n_seg; ++s) {
    if (len[s] < 0 || len[s] > 4096) { snprintf(TEST_ERR, 512, "attention_plan: segment %d has %d rows", s, len[s]); return CZC_ERR_ARG; }
    off[s + 1] = off[s] + len[s];
  }
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < K; ++k) {
      const int s = B + b * K + k;
      poff[s] = off[b]; plen[s] = len[b];
      imax[b] = std::max(imax[b], len[s]);
    }
    max_own = std::max(max_own, imax[b]);
    max_keys = std::max(max_keys, len[b] + imax[b]);
  }
  const size_t rows = off[n_seg], Hd = (size_t)heads * 64, es = prec_bytes(precision);
  const size_t qrow = 3 * Hd * es, orow = Hd * es, all = rows + 2 * GR;
  DevPool pool;
  unsigned char* dq = (unsigned char*)pool.alloc(all * qrow); T_PTR(dq);
  unsigned char* dout = (unsigned char*)pool.alloc(all * orow); T_PTR(dout);
  {  // guard rows of qkv: quiet NaNs of the operand type (fp16 planes for the split type)
    std::vector<uint32_t> nan((size_t)GR * qrow / 4,
                              precision == PREC_F32 ? 0x7fc00000u : precision == PREC_BF16 ? 0x7fc07fc0u : 0x7e007e00u);
    T_HIP(hipMemcpy(dq, nan.data(), (size_t)GR * qrow, hipMemcpyHostToDevice));
    T_HIP(hipMemcpy(dq + (GR + rows) * qrow, nan.data(), (size_t)GR * qrow, hipMemcpyHostToDevice));
  }
  if (rows) {
    float* f = (float*)pool.up(qkv, rows * 3 * Hd * 4); T_PTR(f);
    if (precision == PREC_F32) T_HIP(hipMemcpy(dq + GR * qrow, f, rows * qrow, hipMemcpyDeviceToDevice));
    else T_CHECK(launch_convert(precision, f, dq + GR * qrow, (long)(rows * 3 * Hd), nullptr));
  }
  T_HIP(hipMemset(dout, 0x5a, all * orow));
  int* doff = (int*)pool.up(off.data(), (size_t)(n_seg + 1) * 4); T_PTR(doff);
  int* dlen = (int*)pool.up(len.data(), (size_t)n_seg * 4); T_PTR(dlen);
  int* dpoff = (int*)pool.up(poff.data(), (size_t)n_seg * 4); T_PTR(dpoff);
  int* dplen = (int*)pool.up(plen.data(), (size_t)n_seg * 4); T_PTR(dplen);
  int* dimax = (int*)pool.up(imax.data(), (size_t)B * 4); T_PTR(dimax);
  T_HIP(hipDeviceSynchronize());
  SegTable tab{dpoff, dplen, doff, dlen, n_seg, 0};
  tab.img_max = pass_img_max ? dimax : nullptr;
  const void* q0 = dq + GR * qrow;
  void* o0 = dout + GR * orow;
  int rc;
  if (kernel == 0) {
    rc = launch_attention(precision, q0, tab, max_keys, heads, 1, scale, o0, nullptr);
  } else {
    const int saved = g_use_attention_image;
    g_use_attention_image = kernel == 2 ? 2 : 0;
    rc = half ? launch_attention_shared(q0, tab, B, K, max_own, max_keys, heads, scale, o0, nullptr, precision == PREC_F16)
              : launch_attention_shared_split(q0, tab, B, K, max_own, max_keys, heads, scale, o0, nullptr);
    g_use_attention_image = saved;
  }
  if (rc > 0) return rc;
  T_HIP(hipDeviceSynchronize());
  T_CHECK(down_act(pool, precision, dout, all * Hd, out));
  return rc < 0 ? CZC_TEST_REFUSED : 0;
}

namespace {
// the host-given shared-prefix plan of czc_test_attention_plan, uploaded: tables, sizes, and the NaN pattern of the operand type
struct HostPlan {
  std::vector<int> len, off, poff, plen, imax;
  int n_seg = 0, max_own = 0, max_keys = 0;
  size_t rows = 0;
  SegTable tab{};
  int build(DevPool& pool, const char* who, int B, int K, const int32_t* trunk_len, const int32_t* own_len) {
    n_seg = B + B * K;
    len = std::vector<int>(n_seg); off = std::vector<int>(n_seg + 1, 0); poff = std::vector<int>(n_seg, 0); plen = std::vector<int>(n_seg, 0);
    imax = std::vector<int>(B, 0);
    for (int b = 0; b < B; ++b) len[b] = trunk_len[b];
    for (int i = 0; i < B * K; ++i) len[B + i] = own_len[i];
    for (int s = 0; s < n_seg; ++s) {
      if (len[s] < 0 || len[s] > 4096) { snprintf(TEST_ERR, 512, "%s: segment %d has %d rows", who, s, len[s]); return CZC_ERR_ARG; }
      off[s + 1] = off[s] + len[s];
    }
    for (int b = 0; b < B; ++b) {
      for (int k = 0; k < K; ++k) {
        const int s = B + b * K + k;
        poff[s] = off[b]; plen[s] = len[b];
        imax[b] = std::max(imax[b], len[s]);
      }
      max_own = std::max(max_own, imax[b]);
      max_keys = std::max(max_keys, len[b] + imax[b]);
    }
    rows = off[n_seg];
    int* doff = (int*)pool.up(off.data(), (size_t)(n_seg + 1) * 4); T_PTR(doff);
    int* dlen = (int*)pool.up(len.data(), (size_t)n_seg * 4); T_PTR(dlen);
    int* dpoff = (int*)pool.up(poff.data(), (size_t)n_seg * 4); T_PTR(dpoff);
    int* dplen = (int*)pool.up(plen.data(), (size_t)n_seg * 4); T_PTR(dplen);
    int* dimax = (int*)pool.up(imax.data(), (size_t)B * 4); T_PTR(dimax);
    tab = SegTable{dpoff, dplen, doff, dlen, n_seg, 0};
    tab.img_max = dimax;
    return 0;
  }
};

// n rows of `row` bytes (fp32 host data, rounded to `precision` on the device) with CZC_TEST_PLAN_GUARD rows of NaNs of the operand
// type in front of and behind them; *rows0 = the first data row
int guarded_operand(DevPool& pool, int precision, const float* src, size_t n, size_t row, unsigned char** rows0) {
  const int GR = CZC_TEST_PLAN_GUARD;
  const size_t per_row = row / prec_bytes(precision);  // elements (fp16 planes for the split type: 0x7e00 twice per element)
  unsigned char* d = (unsigned char*)pool.alloc((n + 2 * GR) * row); T_PTR(d);
  std::vector<uint32_t> nan((size_t)GR * row / 4,
                            precision == PREC_F32 ? 0x7fc00000u : precision == PREC_BF16 ? 0x7fc07fc0u : 0x7e007e00u);
  T_HIP(hipMemcpy(d, nan.data(), (size_t)GR * row, hipMemcpyHostToDevice));
  T_HIP(hipMemcpy(d + (GR + n) * row, nan.data(), (size_t)GR * row, hipMemcpyHostToDevice));
  if (n) {
    float* f = (float*)pool.up(src, n * per_row * 4); T_PTR(f);
    if (precision == PREC_F32) T_HIP(hipMemcpy(d + GR * row, f, n * row, hipMemcpyDeviceToDevice));
    else T_CHECK(launch_convert(precision, f, d + GR * row, (long)(n * per_row), nullptr));
  }
  *rows0 = d + GR * row;
  return 0;
}
}  // namespace

// One launch_attention call on plain segments (no prefix), in the two forms of SegTable the towers use: seq_len given -> own_off /
// own_len tables (BERT ragged; zero-length segments allowed), seq_len null -> the fixed_T form (BERT padded, vision).  max_keys 0:
// the longest segment, else what the caller sizes the kernels' LDS with (must cover the longest segment: the kernels trust it).
// Guards and pre-fills as czc_test_attention_plan.
int czc_test_attention_seq(int precision, int n_seg, const int32_t* seq_len, int fixed_T, int max_keys, int heads, int causal,
                           float scale, const float* qkv, float* out) {
  const bool known = precision == PREC_BF16 || precision == PREC_F16 || precision == PREC_F32 || precision == PREC_F16X3;
  if (!known || n_seg < 0 || n_seg > (1 << 20) || heads < 1 || heads > 64 || (causal != 0 && causal != 1) || max_keys < 0 ||
      (!seq_len && (fixed_T < 0 || fixed_T > 4096))) {
    snprintf(TEST_ERR, 512, "attention_seq: precision %d n_seg %d fixed_T %d max_keys %d heads %d causal %d", precision, n_seg, fixed_T,
             max_keys, heads, causal);
    return CZC_ERR_ARG;
  }
  const int GR = CZC_TEST_PLAN_GUARD;
  std::vector<int> off((size_t)n_seg + 1, 0);
  int longest = 0;
  for (int s = 0; s < n_seg; ++s) {
    const int len = seq_len ? seq_len[s] : fixed_T;
    if (len < 0 || len > 4096) { snprintf(TEST_ERR, 512, "attention_seq: segment %d has %d rows", s, len); return CZC_ERR_ARG; }
    off[s + 1] = off[s] + len;
    longest = std::max(longest, len);
  }
  if (max_keys && max_keys < longest) {
    snprintf(TEST_ERR, 512, "attention_seq: max_keys %d below the longest segment (%d rows)", max_keys, longest);
    return CZC_ERR_ARG;
  }
  const size_t rows = off[n_seg], Hd = (size_t)heads * 64, orow = Hd * prec_bytes(precision), all = rows + 2 * GR;
  DevPool pool;
  unsigned char* dq;
  T_CHECK(guarded_operand(pool, precision, qkv, rows, 3 * orow, &dq));
  unsigned char* dout = (unsigned char*)pool.alloc(all * orow); T_PTR(dout);
  T_HIP(hipMemset(dout, 0x5a, all * orow));
  SegTable tab{nullptr, nullptr, nullptr, nullptr, n_seg, fixed_T};
  if (seq_len) {
    int* doff = (int*)pool.up(off.data(), ((size_t)n_seg + 1) * 4); T_PTR(doff);
    int* dlen = (int*)pool.up(seq_len, (size_t)n_seg * 4); T_PTR(dlen);
    tab = SegTable{nullptr, nullptr, doff, dlen, n_seg, 0};
  }
  T_HIP(hipDeviceSynchronize());
  T_CHECK(launch_attention(precision, dq, tab, max_keys ? max_keys : longest, heads, causal, scale, dout + GR * orow, nullptr));
  T_HIP(hipDeviceSynchronize());
  return down_act(pool, precision, dout, all * Hd, out);
}

int czc_test_attention_pooled(int precision, int B, int K, int heads, float scale, const int32_t* trunk_len, const int32_t* own_len,
                              const int32_t* rep, const float* qkv, const float* qc, float* out) {
  if (!(precision == PREC_BF16 || precision == PREC_F16) || B < 1 || K < 1 || heads < 1 || (long)B * K > (1 << 22)) {
    snprintf(TEST_ERR, 512, "attention_pooled: precision %d B %d K %d heads %d", precision, B, K, heads);
    return CZC_ERR_ARG;
  }
  const int GR = CZC_TEST_PLAN_GUARD;
  DevPool pool;
  HostPlan hp;
  T_CHECK(hp.build(pool, "attention_pooled", B, K, trunk_len, own_len));
  const size_t nc = (size_t)B * K, Hd = (size_t)heads * 64, orow = Hd * 2;
  for (size_t i = 0; i < nc; ++i)
    if (rep[i] < 0 || rep[i] >= K || rep[rep[i] + (i / K) * K] != rep[i]) { snprintf(TEST_ERR, 512, "attention_pooled: rep[%zu] = %d", i, rep[i]); return CZC_ERR_ARG; }
  unsigned char *dq, *dqc;
  T_CHECK(guarded_operand(pool, precision, qkv, hp.rows, 3 * orow, &dq));
  T_CHECK(guarded_operand(pool, precision, qc, nc, orow, &dqc));
  unsigned char* dout = (unsigned char*)pool.alloc((nc + 2 * GR) * orow); T_PTR(dout);
  T_HIP(hipMemset(dout, 0x5a, (nc + 2 * GR) * orow));
  int* dpidx = (int*)pool.up(rep, nc * 4); T_PTR(dpidx);
  T_HIP(hipDeviceSynchronize());
  const int saved = g_use_attention_image;
  g_use_attention_image = 2;
  const int rc = HK().attention_image_pooled(dq, dqc, hp.tab, dpidx, B, K, hp.max_own, hp.max_keys, heads, scale, dout + GR * orow, nullptr,
                                             precision == PREC_F16);
  g_use_attention_image = saved;
  if (rc) return rc;
  T_HIP(hipDeviceSynchronize());
  T_CHECK(down_act(pool, precision, dout, (nc + 2 * GR) * Hd, out));
  return 0;
}

int czc_test_attention_mapped(int precision, int B, int K, int heads, float scale, const int32_t* trunk_len, const int32_t* own_len,
                              const int32_t* rowmap, int n_rows, const float* qkv, float* out) {
  if (!(precision == PREC_BF16 || precision == PREC_F16) || B < 1 || K < 1 || heads < 1 || (long)B * K > (1 << 22) || n_rows < 1) {
    snprintf(TEST_ERR, 512, "attention_mapped: precision %d B %d K %d heads %d rows %d", precision, B, K, heads, n_rows);
    return CZC_ERR_ARG;
  }
  const int GR = CZC_TEST_PLAN_GUARD;
  DevPool pool;
  HostPlan hp;
  T_CHECK(hp.build(pool, "attention_mapped", B, K, trunk_len, own_len));
  const size_t Hd = (size_t)heads * 64, orow = Hd * 2, all = hp.rows + 2 * GR;
  for (size_t r = 0; r < hp.rows; ++r)
    if (rowmap[r] < 0 || rowmap[r] >= n_rows) { snprintf(TEST_ERR, 512, "attention_mapped: rowmap[%zu] = %d", r, rowmap[r]); return CZC_ERR_ARG; }
  unsigned char* dq;
  T_CHECK(guarded_operand(pool, precision, qkv, (size_t)n_rows, 3 * orow, &dq));
  unsigned char* dout = (unsigned char*)pool.alloc(all * orow); T_PTR(dout);
  T_HIP(hipMemset(dout, 0x5a, all * orow));
  int* dmap = (int*)pool.up(rowmap, hp.rows * 4); T_PTR(dmap);
  T_HIP(hipDeviceSynchronize());
  const int saved = g_use_attention_image;
  g_use_attention_image = 2;
  const int rc = HK().attention_shared_mapped(dq, n_rows, dmap, hp.tab, B, K, hp.max_own, hp.max_keys, heads, scale, dout + GR * orow, nullptr,
                                              precision == PREC_F16);
  g_use_attention_image = saved;
  if (rc) return rc;
  T_HIP(hipDeviceSynchronize());
  T_CHECK(down_act(pool, precision, dout, all * Hd, out));
  return 0;
}

int czc_test_layer0_plan(int B, int K, const int32_t* clip_ids, const int32_t* clip_len, int dedup, int32_t* own_off, int32_t* own_len,
                         int32_t* dcount, int32_t* totals, int M, int32_t* rowmap, int n_dist, int32_t* dist) {
  const int S = B + B * K, bk = B * K;
  DevPool pool;
  int* dids = (int*)pool.up(clip_ids, (size_t)bk * CZC_CLIP_MAX_LEN * 4); T_PTR(dids);
  int* dlen = (int*)pool.up(clip_len, (size_t)bk * 4); T_PTR(dlen);
  Guarded own, pre, src, pos0, ooff, poff, eidx, grep, imax, tot, dcnt, gmap, gdist;
  T_CHECK(own.make(pool, S)); T_CHECK(pre.make(pool, S)); T_CHECK(src.make(pool, S)); T_CHECK(pos0.make(pool, S));
  T_CHECK(ooff.make(pool, S + 1)); T_CHECK(poff.make(pool, S)); T_CHECK(eidx.make(pool, bk)); T_CHECK(grep.make(pool, bk));
  T_CHECK(imax.make(pool, B)); T_CHECK(tot.make(pool, 12)); T_CHECK(dcnt.make(pool, B));
  T_CHECK(gmap.make(pool, M > 0 ? M : 1)); T_CHECK(gdist.make(pool, n_dist > 0 ? n_dist : 1));
  int* t = tot.p<int>();
  T_HIP(hipMemset(t, 0, 48));
  int* r = dedup ? grep.p<int>() : nullptr;
  T_CHECK(launch_prefix_plan(dids, dlen, B, K, 1, own.p<int>(), pre.p<int>(), src.p<int>(), pos0.p<int>(), t + 3, imax.p<int>(), nullptr, r, t + 5));
  T_CHECK(HK().layer0_count(dids, own.p<int>(), pre.p<int>(), B, K, dcnt.p<int>(), t + 8, nullptr));
  T_CHECK(launch_scan(own.p<int>(), S, ooff.p<int>(), t, nullptr));
  T_CHECK(launch_prefix_finish(ooff.p<int>(), own.p<int>(), B, K, poff.p<int>(), eidx.p<int>(), t + 6, nullptr, r));
  if (M > 0 && n_dist > 0)  // second call of the test, with the sizes the first one returned
    T_CHECK(HK().layer0_map(dids, ooff.p<int>(), own.p<int>(), pre.p<int>(), dcnt.p<int>(), B, K, gmap.p<int>(), gdist.p<int>(), nullptr));
  T_HIP(hipDeviceSynchronize());
  T_CHECK(ooff.down(own_off)); T_CHECK(own.down(own_len)); T_CHECK(dcnt.down(dcount)); T_CHECK(tot.down(totals));
  T_CHECK(gmap.down(rowmap)); T_CHECK(gdist.down(dist));
  return 0;
}

int czc_test_text_tower(void* engine, int B, int K, const int32_t* clip_ids, const int32_t* clip_len, float* feat, int32_t* n_dup) {
  return HK().text_tower(engine, clip_ids, clip_len, B, K, feat, n_dup);
}

int czc_test_topk(int B, int V, int K, const float* logits, const float* mask, float temperature, int dot_id,
                  int dot_allowed, float* probs, int32_t* idxs, int32_t* cand) {
  DevPool pool;
  float* dl = (float*)pool.up(logits, (size_t)B * V * 4); T_PTR(dl);
  float* dm = (float*)pool.up(mask, (size_t)V * 4); T_PTR(dm);
  float* dp = (float*)pool.alloc((size_t)B * K * 4); T_PTR(dp);
  int* di = (int*)pool.alloc((size_t)B * K * 4); T_PTR(di);
  int* dc = (int*)pool.alloc((size_t)B * K * 4); T_PTR(dc);
  T_CHECK(launch_softmax_mask_topk(dl, B, V, K, dm, temperature, dot_id, dot_allowed, dp, di, dc, nullptr));
  T_HIP(hipDeviceSynchronize());
  T_HIP(hipMemcpy(probs, dp, (size_t)B * K * 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(idxs, di, (size_t)B * K * 4, hipMemcpyDeviceToHost));
  if (cand) T_HIP(hipMemcpy(cand, dc, (size_t)B * K * 4, hipMemcpyDeviceToHost));
  return 0;
}

int czc_test_bridge(const czc_bridge_tables* t, const czc_config* cfg, int n_rows, int T, const int32_t* rows,
                    int32_t* clip_ids, int32_t* clip_len) {
  (void)cfg;
  DevPool pool;
  BridgeDev bd;
  T_CHECK(bridge_tables_dev(pool, t, bd));
  int* drows = (int*)pool.up(rows, (size_t)n_rows * T * 4); T_PTR(drows);
  int* dids = (int*)pool.alloc((size_t)n_rows * CZC_CLIP_MAX_LEN * 4); T_PTR(dids);
  int* dlen = (int*)pool.alloc((size_t)n_rows * 4); T_PTR(dlen);
  int* dovf = (int*)pool.alloc(4); T_PTR(dovf);
  T_HIP(hipMemset(dovf, 0, 4));
  PosDev nopos{nullptr, nullptr, 0};
  T_CHECK(launch_bridge(bd, drows, n_rows, T, -1, nullptr, 1, nullptr, nullptr, nullptr, 0, nopos, dids, dlen, nullptr, nullptr, dovf, nullptr));
  T_HIP(hipDeviceSynchronize());
  int ovf = 0;
  T_HIP(hipMemcpy(&ovf, dovf, 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(clip_ids, dids, (size_t)n_rows * CZC_CLIP_MAX_LEN * 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(clip_len, dlen, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
  if (ovf) { snprintf(TEST_ERR, 512, "bridge overflow on %d rows", ovf); return CZC_ERR_OVERFLOW; }
  return 0;
}

int czc_test_combine(int B, int K, int D, const float* text_feat, const float* img_embeds, float logit_scale,
                     const float* probs, const float* senti_raw, const float* repeats, const czc_hyper* hp,
                     float* clip_score, float* clip_ref, float* final_score, int32_t* best) {
  DevPool pool;
  const size_t bk = (size_t)B * K;
  float* dt = (float*)pool.up(text_feat, bk * D * 4); T_PTR(dt);
  float* di = (float*)pool.up(img_embeds, (size_t)B * D * 4); T_PTR(di);
  float* din = (float*)pool.alloc((size_t)B * D * 4); T_PTR(din);
  float* dp = (float*)pool.up(probs, bk * 4); T_PTR(dp);
  float* ds = senti_raw ? (float*)pool.up(senti_raw, bk * 4) : nullptr;
  float* dr = repeats ? (float*)pool.up(repeats, bk * 4) : nullptr;
  int* dcand = (int*)pool.alloc(bk * 4); T_PTR(dcand);
  T_HIP(hipMemset(dcand, 0, bk * 4));
  float* o1 = (float*)pool.alloc(bk * 4); float* o2 = (float*)pool.alloc(bk * 4); float* o3 = (float*)pool.alloc(bk * 4);
  int* ob = (int*)pool.alloc((size_t)B * 4); float* oc = (float*)pool.alloc((size_t)B * 4);
  T_PTR(o1); T_PTR(o2); T_PTR(o3); T_PTR(ob); T_PTR(oc);
  T_CHECK(launch_l2_normalize(di, B, D, din, nullptr));
  CombineArgs a;
  a.text_feat = dt; a.img_n = din; a.logit_scale_exp = expf(logit_scale); a.probs = dp; a.cand = dcand;
  a.senti_raw = ds; a.repeats = dr; a.alpha = hp->alpha; a.beta = hp->beta; a.gamma = hp->gamma;
  a.use_senti = (ds && (dr || hp->control == 2)) ? hp->control : 0; a.B = B; a.K = K; a.D = D; a.clip_score = o1; a.clip_ref = o2;
  a.final_score = o3; a.best = ob; a.best_cos = oc; a.inp = nullptr; a.T = 0; a.gen_idx = 0;
  T_CHECK(launch_combine(a, nullptr));
  T_HIP(hipDeviceSynchronize());
  T_HIP(hipMemcpy(clip_score, o1, bk * 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(clip_ref, o2, bk * 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(final_score, o3, bk * 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(best, ob, (size_t)B * 4, hipMemcpyDeviceToHost));
  return 0;
}

int czc_test_combine_draw(int B, int K, int D, const float* text_feat, const float* img_embeds, float logit_scale,
                          const float* probs, const float* senti_raw, const float* repeats, const czc_hyper* hp,
                          const czc_draw* draw, uint32_t step, float* final_score, int32_t* best) {
  DevPool pool;
  const size_t bk = (size_t)B * K;
  float* dt = (float*)pool.up(text_feat, bk * D * 4); T_PTR(dt);
  float* di = (float*)pool.up(img_embeds, (size_t)B * D * 4); T_PTR(di);
  float* din = (float*)pool.alloc((size_t)B * D * 4); T_PTR(din);
  float* dp = (float*)pool.up(probs, bk * 4); T_PTR(dp);
  float* ds = senti_raw ? (float*)pool.up(senti_raw, bk * 4) : nullptr;
  float* dr = repeats ? (float*)pool.up(repeats, bk * 4) : nullptr;
  int* dcand = (int*)pool.alloc(bk * 4); T_PTR(dcand);
  T_HIP(hipMemset(dcand, 0, bk * 4));
  float* o1 = (float*)pool.alloc(bk * 4); float* o2 = (float*)pool.alloc(bk * 4); float* o3 = (float*)pool.alloc(bk * 4);
  int* ob = (int*)pool.alloc((size_t)B * 4); float* oc = (float*)pool.alloc((size_t)B * 4);
  T_PTR(o1); T_PTR(o2); T_PTR(o3); T_PTR(ob); T_PTR(oc);
  static_assert(sizeof(RowDraw) == sizeof(czc_draw), "RowDraw is czc_draw as the kernels read it");
  RowDraw* dd = (RowDraw*)pool.up(draw, (size_t)B * sizeof(czc_draw)); T_PTR(dd);
  int* dcol = (int*)pool.alloc((size_t)B * 4); T_PTR(dcol);  // the drawing instantiation is a per-row one; nothing is written back (inp null)
  T_HIP(hipMemset(dcol, 0, (size_t)B * 4));
  T_CHECK(launch_l2_normalize(di, B, D, din, nullptr));
  CombineArgs a;
  a.text_feat = dt; a.img_n = din; a.logit_scale_exp = expf(logit_scale); a.probs = dp; a.cand = dcand;
  a.senti_raw = ds; a.repeats = dr; a.alpha = hp->alpha; a.beta = hp->beta; a.gamma = hp->gamma;
  a.use_senti = (ds && (dr || hp->control == 2)) ? hp->control : 0; a.B = B; a.K = K; a.D = D; a.clip_score = o1; a.clip_ref = o2;
  a.final_score = o3; a.best = ob; a.best_cos = oc; a.inp = nullptr; a.T = 0; a.gen_idx = 0;
  a.gen_rows = dcol; a.draw_rows = dd; a.draw_step = step;
  T_CHECK(launch_combine(a, nullptr));
  T_HIP(hipDeviceSynchronize());
  T_HIP(hipMemcpy(final_score, o3, bk * 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(best, ob, (size_t)B * 4, hipMemcpyDeviceToHost));
  return 0;
}

// ---- the integer and selection side of the screen-then-refine engine, one launcher chain at a time ------------------------------
// Every output is a Guarded buffer: the caller's arrays hold CZC_TEST_GUARD + n + CZC_TEST_GUARD words.

int czc_test_scan(int n, const int32_t* len, int32_t* off, int32_t* totals) {
  if (n < 1) { snprintf(TEST_ERR, 512, "scan: n = %d", n); return CZC_ERR_ARG; }
  DevPool pool;
  int* dlen = (int*)pool.up(len, (size_t)n * 4); T_PTR(dlen);
  Guarded goff, gtot;
  T_CHECK(goff.make(pool, (size_t)n + 1)); T_CHECK(gtot.make(pool, 2));
  T_CHECK(launch_scan(dlen, n, goff.p<int>(), gtot.p<int>(), nullptr));
  T_HIP(hipDeviceSynchronize());
  T_CHECK(goff.down(off));
  return gtot.down(totals);
}

// clip_plan of engine.hip: launch_prefix_plan -> launch_scan over the B + B*K segment slots -> launch_prefix_finish on the eight
// pre-zeroed totals words ([0] rows, [1] longest segment, [3] longest sequence, [4] longest branch, [5] duplicates, [6] trunk
// rows, [7] causal pairs).  dedup 0: the kernels get no rep table and `rep` keeps the pattern.
int czc_test_prefix_plan(int B, int K, int share, int dedup, const int32_t* clip_ids, const int32_t* clip_len, int32_t* own_len,
                         int32_t* pre_len, int32_t* seg_src, int32_t* seg_pos0, int32_t* own_off, int32_t* pre_off, int32_t* eos_idx,
                         int32_t* rep, int32_t* img_max, int32_t* totals) {
  if (B < 1 || K < 1 || (long)B * K > (1 << 22)) { snprintf(TEST_ERR, 512, "prefix_plan: B %d K %d", B, K); return CZC_ERR_ARG; }
  const size_t bk = (size_t)B * K, S = B + bk;
  DevPool pool;
  int* dids = (int*)pool.up(clip_ids, bk * CZC_CLIP_MAX_LEN * 4); T_PTR(dids);
  int* dlen = (int*)pool.up(clip_len, bk * 4); T_PTR(dlen);
  Guarded own, pre, src, pos0, ooff, poff, eidx, grep, imax, tot;
  T_CHECK(own.make(pool, S)); T_CHECK(pre.make(pool, S)); T_CHECK(src.make(pool, S)); T_CHECK(pos0.make(pool, S));
  T_CHECK(ooff.make(pool, S + 1)); T_CHECK(poff.make(pool, S)); T_CHECK(eidx.make(pool, bk)); T_CHECK(grep.make(pool, bk));
  T_CHECK(imax.make(pool, B)); T_CHECK(tot.make(pool, 8));
  T_CHECK(tot.zero(8));
  int* t = tot.p<int>();
  int* r = dedup ? grep.p<int>() : nullptr;
  T_CHECK(launch_prefix_plan(dids, dlen, B, K, share, own.p<int>(), pre.p<int>(), src.p<int>(), pos0.p<int>(), t + 3, imax.p<int>(), nullptr, r, t + 5));
  T_CHECK(launch_scan(own.p<int>(), (int)S, ooff.p<int>(), t, nullptr));
  T_CHECK(launch_prefix_finish(ooff.p<int>(), own.p<int>(), B, K, poff.p<int>(), eidx.p<int>(), t + 6, nullptr, r));
  T_HIP(hipDeviceSynchronize());
  T_CHECK(own.down(own_len)); T_CHECK(pre.down(pre_len)); T_CHECK(src.down(seg_src)); T_CHECK(pos0.down(seg_pos0));
  T_CHECK(ooff.down(own_off)); T_CHECK(poff.down(pre_off)); T_CHECK(eidx.down(eos_idx)); T_CHECK(grep.down(rep));
  T_CHECK(imax.down(img_max));
  return tot.down(totals);
}

// form 0: launch_refine_select (theta, beta); 1: launch_refine_select_rows (theta_base, scale, hyper [B]); 2:
// launch_refine_select_draw (draw [B]; hyper [B] or NULL: the scalar theta / beta).  gated: the two pre-zeroed counters.
int czc_test_refine_select(int form, int B, int K, const float* clip_score, const float* final_score, float theta, float theta_base,
                           float scale, int m_samples, float gate_h, float beta, int need_cos, const czc_hyper* hyper,
                           const czc_draw* draw, int32_t* gated, int32_t* kind, int32_t* list, int32_t* count) {
  static_assert(sizeof(RowHyper) == sizeof(czc_hyper), "RowHyper is czc_hyper as the kernels read it");
  if (form < 0 || form > 2 || B < 1 || K < 1 || (form == 1 && !hyper) || (form == 2 && !draw) || (form == 0 && (hyper || draw))) {
    snprintf(TEST_ERR, 512, "refine_select: form %d B %d K %d", form, B, K);
    return CZC_ERR_ARG;
  }
  const size_t bk = (size_t)B * K;
  DevPool pool;
  float* dcs = (float*)pool.up(clip_score, bk * 4); T_PTR(dcs);
  float* dfs = (float*)pool.up(final_score, bk * 4); T_PTR(dfs);
  RowHyper* dh = nullptr;
  RowDraw* dd = nullptr;
  if (hyper) { dh = (RowHyper*)pool.up(hyper, (size_t)B * sizeof(czc_hyper)); T_PTR(dh); }
  if (draw) { dd = (RowDraw*)pool.up(draw, (size_t)B * sizeof(czc_draw)); T_PTR(dd); }
  Guarded gg, gk, gl, gc;
  T_CHECK(gg.make(pool, 2)); T_CHECK(gk.make(pool, bk)); T_CHECK(gl.make(pool, bk)); T_CHECK(gc.make(pool, B));
  T_CHECK(gg.zero(2));
  if (form == 0)
    T_CHECK(launch_refine_select(dcs, dfs, B, K, theta, m_samples, gate_h, beta, need_cos, gg.p<int>(), gk.p<int>(), gl.p<int>(), gc.p<int>(), nullptr));
  else if (form == 1)
    T_CHECK(launch_refine_select_rows(dcs, dfs, B, K, theta_base, scale, m_samples, gate_h, dh, need_cos, gg.p<int>(), gk.p<int>(), gl.p<int>(),
                                      gc.p<int>(), nullptr));
  else
    T_CHECK(launch_refine_select_draw(dcs, dfs, B, K, theta, theta_base, scale, m_samples, gate_h, beta, dh, dd, need_cos, gg.p<int>(), gk.p<int>(),
                                      gl.p<int>(), gc.p<int>(), nullptr));
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gg.down(gated)); T_CHECK(gk.down(kind)); T_CHECK(gl.down(list));
  return gc.down(count);
}

// the plan of the refine pass as step_phase_b queues it: 16 totals words and own_len [B + B*K] zeroed, launch_scan(count)
// (totals[8] = R, [9] = Kr) -> launch_refine_plan -> launch_scan(own_len) (totals[0] = rows) -> launch_refine_finish.
// trunk_len [B]: the prefix lengths of the screening plan.
int czc_test_refine_plan(int B, int K, const int32_t* clip_len, const int32_t* trunk_len, const int32_t* list, const int32_t* count,
                         int32_t* count_off, int32_t* own_len, int32_t* pre_len, int32_t* seg_src, int32_t* seg_pos0, int32_t* own_off,
                         int32_t* pre_off, int32_t* rlist, int32_t* eos_idx, int32_t* img_max, int32_t* totals) {
  if (B < 1 || K < 1 || (long)B * K > (1 << 22)) { snprintf(TEST_ERR, 512, "refine_plan: B %d K %d", B, K); return CZC_ERR_ARG; }
  for (int b = 0; b < B; ++b)
    if (count[b] < 0 || count[b] > K) { snprintf(TEST_ERR, 512, "refine_plan: count[%d] = %d", b, count[b]); return CZC_ERR_ARG; }
  const size_t bk = (size_t)B * K, S = B + bk;
  DevPool pool;
  int* dlen = (int*)pool.up(clip_len, bk * 4); T_PTR(dlen);
  int* dtl = (int*)pool.up(trunk_len, (size_t)B * 4); T_PTR(dtl);
  int* dlist = (int*)pool.up(list, bk * 4); T_PTR(dlist);
  int* dcnt = (int*)pool.up(count, (size_t)B * 4); T_PTR(dcnt);
  Guarded coff, own, pre, src, pos0, ooff, poff, rl, eidx, imax, tot;
  T_CHECK(coff.make(pool, (size_t)B + 1)); T_CHECK(own.make(pool, S)); T_CHECK(pre.make(pool, S)); T_CHECK(src.make(pool, S));
  T_CHECK(pos0.make(pool, S)); T_CHECK(ooff.make(pool, S + 1)); T_CHECK(poff.make(pool, S)); T_CHECK(rl.make(pool, bk));
  T_CHECK(eidx.make(pool, bk)); T_CHECK(imax.make(pool, B)); T_CHECK(tot.make(pool, 16));
  T_CHECK(tot.zero(16));
  T_CHECK(own.zero(S));
  int* t = tot.p<int>();
  T_CHECK(launch_scan(dcnt, B, coff.p<int>(), t + 8, nullptr));
  T_CHECK(launch_refine_plan(dlen, dtl, dlist, dcnt, coff.p<int>(), t + 9, B, K, own.p<int>(), pre.p<int>(), src.p<int>(), pos0.p<int>(),
                             rl.p<int>(), t + 3, imax.p<int>(), nullptr));
  T_CHECK(launch_scan(own.p<int>(), (int)S, ooff.p<int>(), t, nullptr));
  T_CHECK(launch_refine_finish(ooff.p<int>(), own.p<int>(), dcnt, coff.p<int>(), t + 9, B, K, poff.p<int>(), eidx.p<int>(), nullptr));
  T_HIP(hipDeviceSynchronize());
  T_CHECK(coff.down(count_off)); T_CHECK(own.down(own_len)); T_CHECK(pre.down(pre_len)); T_CHECK(src.down(seg_src));
  T_CHECK(pos0.down(seg_pos0)); T_CHECK(ooff.down(own_off)); T_CHECK(poff.down(pre_off)); T_CHECK(rl.down(rlist));
  T_CHECK(eidx.down(eos_idx)); T_CHECK(imax.down(img_max));
  return tot.down(totals);
}

// launch_refine_cosine on n_rows_max compact feature rows of which the first n_rows count (the engine's R, read on the device):
// text_feat [n_rows_max, D], img [B, D] (normalised here by launch_l2_normalize, as czc_test_combine does), rlist [n_rows_max]
// (flat candidate b*K + k of each row) -> cos_out [B*K], nonfinite (8 pre-zeroed words; [0] is the cosine check's flag).
int czc_test_refine_cosine(int n_rows_max, int n_rows, int B, int K, int D, const float* text_feat, const float* img_embeds,
                           const int32_t* rlist, float* cos_out, int32_t* nonfinite) {
  if (n_rows_max < 1 || n_rows < 0 || n_rows > n_rows_max || B < 1 || K < 1 || D < 1) {
    snprintf(TEST_ERR, 512, "refine_cosine: rows %d of %d B %d K %d D %d", n_rows, n_rows_max, B, K, D);
    return CZC_ERR_ARG;
  }
  for (int r = 0; r < n_rows; ++r)
    if (rlist[r] < 0 || rlist[r] >= B * K) { snprintf(TEST_ERR, 512, "refine_cosine: rlist[%d] = %d", r, rlist[r]); return CZC_ERR_ARG; }
  DevPool pool;
  float* dt = (float*)pool.up(text_feat, (size_t)n_rows_max * D * 4); T_PTR(dt);
  float* di = (float*)pool.up(img_embeds, (size_t)B * D * 4); T_PTR(di);
  float* din = (float*)pool.alloc((size_t)B * D * 4); T_PTR(din);
  int* drl = (int*)pool.up(rlist, (size_t)n_rows_max * 4); T_PTR(drl);
  int* dn = (int*)pool.up(&n_rows, 4); T_PTR(dn);
  Guarded gcos, gnf;
  T_CHECK(gcos.make(pool, (size_t)B * K)); T_CHECK(gnf.make(pool, 8));
  T_CHECK(gnf.zero(8));
  T_CHECK(launch_l2_normalize(di, B, D, din, nullptr));
  T_CHECK(launch_refine_cosine(dt, din, drl, dn, n_rows_max, K, D, gcos.p<float>(), gnf.p<int>(), nullptr));
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gcos.down(cos_out));
  return gnf.down(nonfinite);
}

// The final combine of the refine engine: the screening cosines cos_in [B*K] enter through clip_ref (text_feat null), candidates
// marked in refine_kind take refine_cos.  nonfinite: 8 pre-zeroed words ([1] the float bits of the guard deviation, [2] trips).
int czc_test_combine_refine(int B, int K, float logit_scale, const float* cos_in, const float* probs, const czc_hyper* hp,
                            const int32_t* refine_kind, const float* refine_cos, float refine_guard, float* clip_score, float* clip_ref,
                            float* final_score, int32_t* best, float* best_cos, int32_t* nonfinite) {
  if (B < 1 || K < 1) { snprintf(TEST_ERR, 512, "combine_refine: B %d K %d", B, K); return CZC_ERR_ARG; }
  DevPool pool;
  const size_t bk = (size_t)B * K;
  float* dp = (float*)pool.up(probs, bk * 4); T_PTR(dp);
  int* dk = (int*)pool.up(refine_kind, bk * 4); T_PTR(dk);
  float* drc = (float*)pool.up(refine_cos, bk * 4); T_PTR(drc);
  int* dcand = (int*)pool.alloc(bk * 4); T_PTR(dcand);
  T_HIP(hipMemset(dcand, 0, bk * 4));
  Guarded o1, o2, o3, ob, oc, gnf;
  T_CHECK(o1.make(pool, bk)); T_CHECK(o2.make(pool, bk)); T_CHECK(o3.make(pool, bk)); T_CHECK(ob.make(pool, B)); T_CHECK(oc.make(pool, B));
  T_CHECK(gnf.make(pool, 8));
  T_CHECK(gnf.zero(8));
  T_CHECK(o2.fill(cos_in));
  CombineArgs a;
  a.text_feat = nullptr; a.img_n = nullptr; a.logit_scale_exp = expf(logit_scale); a.probs = dp; a.cand = dcand;
  a.senti_raw = nullptr; a.repeats = nullptr; a.alpha = hp->alpha; a.beta = hp->beta; a.gamma = hp->gamma; a.use_senti = 0;
  a.B = B; a.K = K; a.D = 0; a.clip_score = o1.p<float>(); a.clip_ref = o2.p<float>(); a.final_score = o3.p<float>();
  a.best = ob.p<int>(); a.best_cos = oc.p<float>(); a.inp = nullptr; a.T = 0; a.gen_idx = 0; a.nonfinite = gnf.p<int>();
  a.refine_kind = dk; a.refine_cos = drc; a.refine_guard = refine_guard;
  T_CHECK(launch_combine(a, nullptr));
  T_HIP(hipDeviceSynchronize());
  T_CHECK(o1.down(clip_score)); T_CHECK(o2.down(clip_ref)); T_CHECK(o3.down(final_score)); T_CHECK(ob.down(best)); T_CHECK(oc.down(best_cos));
  return gnf.down(nonfinite);
}

// The rival instantiation of the combine: rows [B] with their own image image_of_row[b] of img_all [n_img, D] (normalised here by
// launch_l2_normalize; the rows' own embeddings are the gathered copy, as in the rows calls) and rival_idx [B, M] into img_all.
// draw NULL: no row draws.  Outputs are Guarded; nonfinite: 8 pre-zeroed words.
int czc_test_combine_rivals(int B, int K, int D, const float* text_feat, const float* img_all, int n_img, const int32_t* image_of_row,
                            const int32_t* rival_idx, int M, const float* delta, float logit_scale, const float* probs,
                            const czc_hyper* hp, const czc_draw* draw, uint32_t step, float* clip_ref, float* disc, float* final_score,
                            int32_t* best, int32_t* nonfinite) {
  if (B < 1 || K < 1 || D < 1 || n_img < 1 || M < 1 || M > CZC_MAX_RIVALS || (long)D * CZC_MAX_RIVALS > CB_RIVAL_FLOATS) {
    snprintf(TEST_ERR, 512, "combine_rivals: B %d K %d D %d n_img %d M %d", B, K, D, n_img, M);
    return CZC_ERR_ARG;
  }
  for (int b = 0; b < B; ++b) {  // what the entry points refuse: nothing out of bounds reaches the kernel
    if (image_of_row[b] < 0 || image_of_row[b] >= n_img) { snprintf(TEST_ERR, 512, "combine_rivals: image_of_row"); return CZC_ERR_ARG; }
    if (hp[b].control != 0) { snprintf(TEST_ERR, 512, "combine_rivals: the hook carries no control scores"); return CZC_ERR_ARG; }
    for (int j = 0; j < M; ++j)
      if (rival_idx[(size_t)b * M + j] < -1 || rival_idx[(size_t)b * M + j] >= n_img) { snprintf(TEST_ERR, 512, "combine_rivals: rival index"); return CZC_ERR_ARG; }
  }
  DevPool pool;
  const size_t bk = (size_t)B * K;
  float* dt = (float*)pool.up(text_feat, bk * D * 4); T_PTR(dt);
  float* di = (float*)pool.up(img_all, (size_t)n_img * D * 4); T_PTR(di);
  float* dall = (float*)pool.alloc((size_t)n_img * D * 4); T_PTR(dall);
  float* din = (float*)pool.alloc((size_t)B * D * 4); T_PTR(din);
  float* dp = (float*)pool.up(probs, bk * 4); T_PTR(dp);
  int* dcand = (int*)pool.alloc(bk * 4); T_PTR(dcand);
  T_HIP(hipMemset(dcand, 0, bk * 4));
  int* driv = (int*)pool.up(rival_idx, (size_t)B * M * 4); T_PTR(driv);
  float* ddel = (float*)pool.up(delta, (size_t)B * 4); T_PTR(ddel);
  static_assert(sizeof(RowHyper) == sizeof(czc_hyper), "RowHyper is czc_hyper as the kernels read it");
  RowHyper* dh = (RowHyper*)pool.up(hp, (size_t)B * sizeof(czc_hyper)); T_PTR(dh);
  std::vector<czc_draw> nodraw((size_t)B, czc_draw{0, 0.f, 0});
  RowDraw* dd = (RowDraw*)pool.up(draw ? draw : nodraw.data(), (size_t)B * sizeof(czc_draw)); T_PTR(dd);
  int* dcol = (int*)pool.alloc((size_t)B * 4); T_PTR(dcol);
  T_HIP(hipMemset(dcol, 0, (size_t)B * 4));
  Guarded o1, o2, o3, od, ob, oc, gnf;
  T_CHECK(o1.make(pool, bk)); T_CHECK(o2.make(pool, bk)); T_CHECK(o3.make(pool, bk)); T_CHECK(od.make(pool, bk));
  T_CHECK(ob.make(pool, B)); T_CHECK(oc.make(pool, B)); T_CHECK(gnf.make(pool, 8));
  T_CHECK(gnf.zero(8));
  T_CHECK(launch_l2_normalize(di, n_img, D, dall, nullptr));
  T_HIP(hipDeviceSynchronize());
  for (int b = 0; b < B; ++b)
    T_HIP(hipMemcpy(din + (size_t)b * D, dall + (size_t)image_of_row[b] * D, (size_t)D * 4, hipMemcpyDeviceToDevice));
  CombineArgs a;
  a.text_feat = dt; a.img_n = din; a.logit_scale_exp = expf(logit_scale); a.probs = dp; a.cand = dcand;
  a.senti_raw = nullptr; a.repeats = nullptr; a.alpha = hp->alpha; a.beta = hp->beta; a.gamma = hp->gamma; a.use_senti = 0;
  a.B = B; a.K = K; a.D = D; a.clip_score = o1.p<float>(); a.clip_ref = o2.p<float>(); a.final_score = o3.p<float>();
  a.best = ob.p<int>(); a.best_cos = oc.p<float>(); a.inp = nullptr; a.T = 0; a.gen_idx = 0; a.nonfinite = gnf.p<int>();
  a.gen_rows = dcol; a.hp_rows = dh; a.draw_rows = dd; a.draw_step = step;
  a.rival_idx = driv; a.M = M; a.rival_delta = ddel; a.img_all = dall; a.n_img = n_img; a.disc = od.p<float>();
  T_CHECK(launch_combine(a, nullptr));
  T_HIP(hipDeviceSynchronize());
  T_CHECK(o2.down(clip_ref)); T_CHECK(od.down(disc)); T_CHECK(o3.down(final_score)); T_CHECK(ob.down(best));
  return gnf.down(nonfinite);
}

}  // extern "C"

// ---- the row, embedding, mover and memo kernels one by one (rowops.hip, ragged.hip, memo.hip, memo_rows.hip) ----------------------
// Every output is a Guarded buffer of 4-byte words and comes back RAW (typed activations as the bytes the kernel stored:
// tests/kernel_hooks.py decodes bf16 / fp16 / split hi + lo planes), so that results can be compared bit for bit.  Every index a
// kernel would follow is checked on the host first: nothing out of bounds reaches a launch.  A launcher that refuses its shape
// (status 1) launches nothing: the hook still returns every output (the untouched pattern) with CZC_TEST_REFUSED.
namespace {
size_t act_words(int prec, size_t n) { return (n * prec_bytes(prec) + 3) / 4; }
int launch_status(int rc) { return rc == 0 ? 0 : rc == 1 ? CZC_TEST_REFUSED : CZC_ERR_HIP; }
bool all_in(const int32_t* v, size_t n, long lo, long hi) {  // lo <= v[i] < hi
  for (size_t i = 0; i < n; ++i) if (v[i] < lo || v[i] >= hi) return false;
  return true;
}
bool prec_known(int p) { return p == PREC_BF16 || p == PREC_F32 || p == PREC_F16X3 || p == PREC_F16; }
#define T_ARG(cond, who) do { if (!(cond)) { snprintf(TEST_ERR, 512, "%s: argument check failed: %s", who, #cond); return CZC_ERR_ARG; } } while (0)
// a Guarded buffer of n words holding host data (null: the pattern)
int guarded_in(DevPool& pool, Guarded& g, const void* src, size_t words) {
  T_CHECK(g.make(pool, words));
  if (src && words) T_CHECK(g.fill(src));
  return 0;
}
}  // namespace

extern "C" {

int czc_test_layernorm_rows(int precision, int M, int H, int n_src, const float* x, const int32_t* row_idx, const float* gamma,
                            const float* beta, float eps, int mode, int32_t* y_act, float* y_f32) {
  const char* who = "layernorm_rows";
  const bool want_act = mode & 1, want_f32 = mode & 2, alias = mode & 4;
  T_ARG(prec_known(precision) && M >= 1 && H >= 1 && H <= 4096 && n_src >= 1 && (want_act || want_f32), who);
  T_ARG(!alias || (want_f32 && !row_idx && n_src == M), who);  // in place: row m reads and writes row m only
  T_ARG(row_idx ? all_in(row_idx, M, 0, n_src) : n_src >= M, who);
  DevPool pool;
  Guarded gx, ga, gf;
  T_CHECK(guarded_in(pool, gx, x, (size_t)n_src * H));
  float* dg = (float*)pool.up(gamma, (size_t)H * 4); T_PTR(dg);
  float* db = (float*)pool.up(beta, (size_t)H * 4); T_PTR(db);
  int* di = row_idx ? (int*)pool.up(row_idx, (size_t)M * 4) : nullptr;
  if (row_idx) T_PTR(di);
  T_CHECK(ga.make(pool, act_words(precision, (size_t)M * H)));
  if (!alias) T_CHECK(gf.make(pool, (size_t)M * H));
  float* yf = !want_f32 ? nullptr : alias ? gx.p<float>() : gf.p<float>();
  const int rc = launch_layernorm(precision, gx.p<float>(), di, dg, db, eps, M, H, want_act ? ga.p<void>() : nullptr, yf, nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(ga.down(y_act));
  T_CHECK((alias ? gx : gf).down(y_f32));
  return launch_status(rc);
}

int czc_test_layernorm_x16_rows(int precision, int M, int H, int n_src, const float* x, const int32_t* row_idx, const float* gamma,
                                const float* beta, float eps, int32_t* y_act) {
  const char* who = "layernorm_x16_rows";
  T_ARG(prec_known(precision) && M >= 1 && H >= 8 && H <= 4096 && H % 8 == 0 && n_src >= 1, who);
  T_ARG(row_idx ? all_in(row_idx, M, 0, n_src) : n_src >= M, who);
  DevPool pool;
  void* dx = up_act(pool, PREC_F16, x, (size_t)n_src * H); T_PTR(dx);
  float* dg = (float*)pool.up(gamma, (size_t)H * 4); T_PTR(dg);
  float* db = (float*)pool.up(beta, (size_t)H * 4); T_PTR(db);
  int* di = row_idx ? (int*)pool.up(row_idx, (size_t)M * 4) : nullptr;
  if (row_idx) T_PTR(di);
  Guarded ga;
  T_CHECK(ga.make(pool, (size_t)M * H / 2));
  T_HIP(hipDeviceSynchronize());
  const int rc = launch_layernorm_x16(precision, dx, di, dg, db, eps, M, H, ga.p<void>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(ga.down(y_act));
  return launch_status(rc);
}

int czc_test_layernorm_splitk(int precision, int nslab, int M, int H, int ld, const float* slabs, const float* bias, const float* resid,
                              int ldr, const float* gamma, const float* beta, float eps, int32_t* y_act, float* y_f32) {
  const char* who = "layernorm_splitk";
  T_ARG(prec_known(precision) && nslab >= 1 && nslab <= 64 && M >= 1 && H >= 1 && H <= 4096 && ld >= H && (!resid || ldr >= H), who);
  DevPool pool;
  float* ds = (float*)pool.up(slabs, (size_t)nslab * M * ld * 4); T_PTR(ds);
  float* dbias = bias ? (float*)pool.up(bias, (size_t)H * 4) : nullptr;
  float* dres = resid ? (float*)pool.up(resid, (size_t)M * ldr * 4) : nullptr;
  if (bias) T_PTR(dbias);
  if (resid) T_PTR(dres);
  float* dg = (float*)pool.up(gamma, (size_t)H * 4); T_PTR(dg);
  float* db = (float*)pool.up(beta, (size_t)H * 4); T_PTR(db);
  Guarded ga, gf;
  T_CHECK(ga.make(pool, act_words(precision, (size_t)M * H))); T_CHECK(gf.make(pool, (size_t)M * H));
  SplitkPending sk;
  sk.slabs = ds; sk.nslab = nslab; sk.slab_stride = (long)M * ld; sk.ld = ld;
  const int rc = HK().layernorm_splitk(precision, sk, dbias, dres, ldr, dg, db, eps, M, H, ga.p<void>(), gf.p<float>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(ga.down(y_act));
  T_CHECK(gf.down(y_f32));
  return launch_status(rc);
}

int czc_test_ln_finalize(int nblk, int M, int ld, const float* part, float eps, float* stat) {
  const char* who = "ln_finalize";
  T_ARG(nblk >= 1 && nblk <= 64 && M >= 1 && ld >= M, who);
  DevPool pool;
  float* dp = (float*)pool.up(part, (size_t)nblk * ld * 8); T_PTR(dp);
  Guarded gs;
  T_CHECK(gs.make(pool, (size_t)M * 2));
  const int rc = launch_ln_finalize(dp, ld, nblk, M, eps, gs.p<float>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gs.down(stat));
  return launch_status(rc);
}

int czc_test_bert_embed(int precision, int B, int T, int H, int V, int n_pos, const int32_t* ids, const float* word, const float* pos,
                        const float* type0, const float* gamma, const float* beta, float eps, int32_t* y_act, float* y_f32) {
  const char* who = "bert_embed";
  T_ARG(prec_known(precision) && B >= 1 && T >= 1 && T <= n_pos && H >= 1 && H <= 4096 && V >= 1 && all_in(ids, (size_t)B * T, 0, V), who);
  DevPool pool;
  int* di = (int*)pool.up(ids, (size_t)B * T * 4); T_PTR(di);
  float* dw = (float*)pool.up(word, (size_t)V * H * 4); T_PTR(dw);
  float* dp = (float*)pool.up(pos, (size_t)n_pos * H * 4); T_PTR(dp);
  float* dt = (float*)pool.up(type0, (size_t)H * 4); T_PTR(dt);
  float* dg = (float*)pool.up(gamma, (size_t)H * 4); T_PTR(dg);
  float* db = (float*)pool.up(beta, (size_t)H * 4); T_PTR(db);
  Guarded ga, gf;
  T_CHECK(ga.make(pool, act_words(precision, (size_t)B * T * H))); T_CHECK(gf.make(pool, (size_t)B * T * H));
  const int rc = HK().bert_embed(precision, di, B, T, H, dw, dp, dt, dg, db, eps, ga.p<void>(), gf.p<float>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(ga.down(y_act));
  T_CHECK(gf.down(y_f32));
  return launch_status(rc);
}

int czc_test_bert_embed_ragged(int precision, int n, int n_id_rows, int ids_stride, int max_T, int H, int V, int n_pos, const int32_t* ids,
                               const int32_t* run, const int32_t* row_off, const int32_t* row_len, int n_out_rows, const float* word,
                               const float* pos, const float* type0, const float* gamma, const float* beta, float eps, int32_t* y_act,
                               float* y_f32) {
  const char* who = "bert_embed_ragged";
  T_ARG(prec_known(precision) && n >= 1 && n_id_rows >= 1 && ids_stride >= 1 && max_T >= 1 && max_T <= n_pos && H >= 1 && H <= 4096 && V >= 1 &&
        n_out_rows >= 1, who);
  T_ARG(all_in(ids, (size_t)n_id_rows * ids_stride, 0, V), who);  // the padding columns too: a wrong read must show as a value
  T_ARG(run ? all_in(run, n, 0, n_id_rows) : n <= n_id_rows, who);
  T_ARG(all_in(row_len, n, 0, (max_T < ids_stride ? max_T : ids_stride) + 1), who);
  for (int b = 0; b < n; ++b) T_ARG(row_off[b] >= 0 && row_off[b] + row_len[b] <= n_out_rows, who);
  DevPool pool;
  int* di = (int*)pool.up(ids, (size_t)n_id_rows * ids_stride * 4); T_PTR(di);
  int* drun = run ? (int*)pool.up(run, (size_t)n * 4) : nullptr;
  if (run) T_PTR(drun);
  int* doff = (int*)pool.up(row_off, (size_t)(n + 1) * 4); T_PTR(doff);
  int* dlen = (int*)pool.up(row_len, (size_t)n * 4); T_PTR(dlen);
  float* dw = (float*)pool.up(word, (size_t)V * H * 4); T_PTR(dw);
  float* dp = (float*)pool.up(pos, (size_t)n_pos * H * 4); T_PTR(dp);
  float* dt = (float*)pool.up(type0, (size_t)H * 4); T_PTR(dt);
  float* dg = (float*)pool.up(gamma, (size_t)H * 4); T_PTR(dg);
  float* db = (float*)pool.up(beta, (size_t)H * 4); T_PTR(db);
  Guarded ga, gf;
  T_CHECK(ga.make(pool, act_words(precision, (size_t)n_out_rows * H))); T_CHECK(gf.make(pool, (size_t)n_out_rows * H));
  const int rc = HK().bert_embed_ragged(precision, di, ids_stride, drun, doff, dlen, n, max_T, H, dw, dp, dt, dg, db, eps, ga.p<void>(),
                                        gf.p<float>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(ga.down(y_act));
  T_CHECK(gf.down(y_f32));
  return launch_status(rc);
}

int czc_test_clip_embed(int mode, int n_seg, int max_len, int H, int n_id_rows, int ids_stride, const int32_t* ids, const int32_t* seg_src,
                        const int32_t* seg_pos0, const int32_t* own_off, const int32_t* own_len, int V, int n_pos, const float* tok,
                        const float* pos, int n_out_rows, float eps, int32_t* x_out, float* stat) {
  const char* who = "clip_embed";
  T_ARG(mode >= 0 && mode <= 2 && n_seg >= 1 && max_len >= 1 && H >= 1 && H <= 4096 && n_id_rows >= 1 && ids_stride >= 1 && V >= 1 && n_pos >= 1 &&
        n_out_rows >= 1, who);
  T_ARG(all_in(ids, (size_t)n_id_rows * ids_stride, 0, V) && all_in(seg_src, n_seg, 0, n_id_rows) && all_in(own_len, n_seg, 0, max_len + 1), who);
  for (int s = 0; s < n_seg; ++s)
    T_ARG(seg_pos0[s] >= 0 && seg_pos0[s] + own_len[s] <= ids_stride && seg_pos0[s] + own_len[s] <= n_pos && own_off[s] >= 0 &&
          own_off[s] + own_len[s] <= n_out_rows, who);
  DevPool pool;
  int* di = (int*)pool.up(ids, (size_t)n_id_rows * ids_stride * 4); T_PTR(di);
  int* dsrc = (int*)pool.up(seg_src, (size_t)n_seg * 4); T_PTR(dsrc);
  int* dp0 = (int*)pool.up(seg_pos0, (size_t)n_seg * 4); T_PTR(dp0);
  int* doff = (int*)pool.up(own_off, (size_t)n_seg * 4); T_PTR(doff);
  int* dlen = (int*)pool.up(own_len, (size_t)n_seg * 4); T_PTR(dlen);
  float* dtok = (float*)pool.up(tok, (size_t)V * H * 4); T_PTR(dtok);
  float* dpos = (float*)pool.up(pos, (size_t)n_pos * H * 4); T_PTR(dpos);
  Guarded gx, gs;
  T_CHECK(gx.make(pool, act_words(mode ? PREC_F16 : PREC_F32, (size_t)n_out_rows * H))); T_CHECK(gs.make(pool, (size_t)n_out_rows * 2));
  const int rc = HK().clip_embed(di, ids_stride, dsrc, dp0, doff, dlen, n_seg, max_len, H, dtok, dpos, gx.p<float>(), nullptr, mode ? 1 : 0,
                                 mode == 2 ? gs.p<float>() : nullptr, eps);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gx.down(x_out));
  T_CHECK(gs.down(stat));
  return launch_status(rc);
}

int czc_test_im2col(int precision, int B, int S, int p, const float* pixels, int32_t* out) {
  const char* who = "im2col";
  T_ARG(prec_known(precision) && B >= 1 && S >= 1 && S <= 1024 && p >= 1 && p <= S, who);
  DevPool pool;
  float* dpix = (float*)pool.up(pixels, (size_t)B * 3 * S * S * 4); T_PTR(dpix);
  Guarded go;
  T_CHECK(go.make(pool, act_words(precision, (size_t)B * (S / p) * (S / p) * 3 * p * p)));
  const int rc = HK().im2col(precision, dpix, B, S, p, go.p<void>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(go.down(out));
  return launch_status(rc);
}

int czc_test_vision_assemble(int B, int P, int H, const float* patch_out, const float* cls, const float* pos, float* x) {
  const char* who = "vision_assemble";
  T_ARG(B >= 1 && P >= 1 && H >= 1, who);
  DevPool pool;
  float* dpo = (float*)pool.up(patch_out, (size_t)B * P * H * 4); T_PTR(dpo);
  float* dcls = (float*)pool.up(cls, (size_t)H * 4); T_PTR(dcls);
  float* dpos = (float*)pool.up(pos, (size_t)(P + 1) * H * 4); T_PTR(dpos);
  Guarded gx;
  T_CHECK(gx.make(pool, (size_t)B * (P + 1) * H));
  const int rc = HK().vision_assemble(dpo, B, P, H, dcls, dpos, gx.p<float>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gx.down(x));
  return launch_status(rc);
}

int czc_test_l2_normalize(int M, int D, const float* x, float* y) {
  const char* who = "l2_normalize";
  T_ARG(M >= 1 && D >= 1, who);
  DevPool pool;
  float* dx = (float*)pool.up(x, (size_t)M * D * 4); T_PTR(dx);
  Guarded gy;
  T_CHECK(gy.make(pool, (size_t)M * D));
  const int rc = launch_l2_normalize(dx, M, D, gy.p<float>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gy.down(y));
  return launch_status(rc);
}

// kind 0: launch_gather_rows_f32 (W floats per row), 1: launch_gather_rows_bytes (W bytes per row, W % 4 == 0 here), 2:
// launch_gather_rows_w32 (W words per row); src: n_src rows, dst: M rows
int czc_test_gather_rows(int kind, int M, int W, int n_src, const int32_t* src, const int32_t* idx, int32_t* dst) {
  const char* who = "gather_rows";
  T_ARG(kind >= 0 && kind <= 2 && M >= 1 && W >= 1 && n_src >= 1 && (kind != 1 || W % 4 == 0) && all_in(idx, M, 0, n_src), who);
  const size_t rw = kind == 1 ? W / 4 : W;
  DevPool pool;
  int* ds = (int*)pool.up(src, (size_t)n_src * rw * 4); T_PTR(ds);
  int* di = (int*)pool.up(idx, (size_t)M * 4); T_PTR(di);
  Guarded gd;
  T_CHECK(gd.make(pool, (size_t)M * rw));
  const int rc = kind == 0   ? HK().gather_rows_f32((const float*)ds, di, M, W, gd.p<float>(), nullptr)
                 : kind == 1 ? HK().gather_rows_bytes(ds, di, M, W, gd.p<void>(), nullptr)
                             : HK().gather_rows_w32(ds, di, M, W, gd.p<void>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gd.down(dst));
  return launch_status(rc);
}

// gen_rows NULL: launch_mask_positions at gen_idx; else launch_mask_positions_rows (a row with gen_rows[b] < 0 is left alone)
int czc_test_mask_positions(int B, int T, int gen_idx, const int32_t* gen_rows, int n_mask, int mask_id, const int32_t* inp, int32_t* inp_out) {
  const char* who = "mask_positions";
  T_ARG(B >= 1 && T >= 1 && n_mask >= 0 && (long)B * n_mask < (1 << 24) && (gen_rows ? all_in(gen_rows, B, -1, 1 << 20) : gen_idx >= 0), who);
  DevPool pool;
  Guarded gi;
  T_CHECK(guarded_in(pool, gi, inp, (size_t)B * T));
  int* dgen = gen_rows ? (int*)pool.up(gen_rows, (size_t)B * 4) : nullptr;
  if (gen_rows) T_PTR(dgen);
  const int rc = gen_rows ? HK().mask_positions_rows(gi.p<int>(), B, T, dgen, n_mask, mask_id, nullptr)
                          : HK().mask_positions(gi.p<int>(), B, T, gen_idx, n_mask, mask_id, nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gi.down(inp_out));
  return launch_status(rc);
}

int czc_test_tie_rows(int R, int T, int G, const int32_t* inp, const int32_t* col, const int32_t* grp_of_row, const int32_t* grp_off,
                      const int32_t* grp_rows, int32_t* inp_out) {
  const char* who = "tie_rows";
  T_ARG(R >= 1 && T >= 1 && G >= 1 && all_in(grp_of_row, R, 0, G) && grp_off[0] == 0, who);
  for (int g = 0; g < G; ++g) T_ARG(grp_off[g + 1] >= grp_off[g] && grp_off[g + 1] <= (1 << 24), who);
  const int n_gr = grp_off[G];
  DevPool pool;
  Guarded gi;
  T_CHECK(guarded_in(pool, gi, inp, (size_t)R * T));
  int* dcol = (int*)pool.up(col, (size_t)R * 4); T_PTR(dcol);
  int* dgor = (int*)pool.up(grp_of_row, (size_t)R * 4); T_PTR(dgor);
  int* dgoff = (int*)pool.up(grp_off, (size_t)(G + 1) * 4); T_PTR(dgoff);
  int* dgr = (int*)pool.up(grp_rows, (size_t)(n_gr ? n_gr : 1) * 4); T_PTR(dgr);
  const int rc = HK().tie_rows(gi.p<int>(), R, T, dcol, dgor, dgoff, dgr, nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gi.down(inp_out));
  return launch_status(rc);
}

// The image memo of czc_generate, as memo_step of engine.hip chains it for one sub-step: launch_memo_check; then (stages != 0), with n =
// tot[0] read back: launch_memo_fill when n < B; nothing more when n == 0; else launch_memo_gather (use_list: the compact batch
// of the listed images; else the whole batch in place, keys only), "the step" (compact row i takes new_rows / new_cos / new_max of
// its image: what the host says the step leaves), launch_memo_scatter.  record 0: no key is written and the entry (ent_*) is not
// passed to the scatter.  In: inp, key [B*T], img_max [2*B], img_n [B*D], new_rows [B*T], new_cos, new_max [B], ent_rows [B*T],
// ent_cos, ent_max, bcos_in [B].  Out (guarded): hit, list [B], tot [4], key_out, inp_out [B*T], bcos_out [B], ent_rows_out [B*T],
// ent_cos_out, ent_max_out [B], inp_c [B*T], img_c [B*D].
int czc_test_memo_chain(int B, int T, int D, int gen_idx, int n_mask, int mask_id, int n_sub, int stages, int use_list, int record,
                        const int32_t* inp, const int32_t* key, const int32_t* img_max, const float* img_n, const int32_t* new_rows,
                        const float* new_cos, const int32_t* new_max, const int32_t* ent_rows, const float* ent_cos, const int32_t* ent_max,
                        const float* bcos_in, int32_t* hit, int32_t* list, int32_t* tot, int32_t* key_out, int32_t* inp_out, float* bcos_out,
                        int32_t* ent_rows_out, float* ent_cos_out, int32_t* ent_max_out, int32_t* inp_c, float* img_c) {
  const char* who = "memo_chain";
  T_ARG(B >= 1 && B <= (1 << 20) && T >= 1 && D >= 1 && gen_idx >= 0 && n_mask >= 0 && n_sub >= 1 && n_sub <= 2, who);
  const size_t bt = (size_t)B * T;
  DevPool pool;
  Guarded ginp, gkey, ghit, glist, gtot, gbcos, grows, gcos, gmax, ginpc, gimgc;
  T_CHECK(guarded_in(pool, ginp, inp, bt)); T_CHECK(guarded_in(pool, gkey, key, bt));
  T_CHECK(ghit.make(pool, B)); T_CHECK(glist.make(pool, B)); T_CHECK(gtot.make(pool, 4));
  T_CHECK(guarded_in(pool, gbcos, bcos_in, B)); T_CHECK(guarded_in(pool, grows, ent_rows, bt)); T_CHECK(guarded_in(pool, gcos, ent_cos, B));
  T_CHECK(guarded_in(pool, gmax, ent_max, B)); T_CHECK(ginpc.make(pool, bt)); T_CHECK(gimgc.make(pool, (size_t)B * D));
  int* dimax = (int*)pool.up(img_max, (size_t)2 * B * 4); T_PTR(dimax);
  int rc = HK().memo_check(ginp.p<int>(), B, T, gen_idx, n_mask, mask_id, gkey.p<int>(), dimax, n_sub, ghit.p<int>(), glist.p<int>(),
                           gtot.p<int>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  if (rc == 0 && stages) {
    int n = 0;
    T_HIP(hipMemcpy(&n, gtot.p<int>(), 4, hipMemcpyDeviceToHost));
    T_ARG(n >= 0 && n <= B, who);
    std::vector<int> hl((size_t)B);
    T_HIP(hipMemcpy(hl.data(), glist.p<int>(), (size_t)B * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) T_ARG(hl[i] >= 0 && hl[i] < B, who);  // a wrong list is reported, never followed
    if (n < B) rc = HK().memo_fill(ghit.p<int>(), B, T, grows.p<int>(), gcos.p<float>(), ginp.p<int>(), gbcos.p<float>(), nullptr);
    if (rc == 0 && n > 0) {
      const bool compact = use_list != 0;
      const int m = compact ? n : B;
      float* dimg = (float*)pool.up(img_n, (size_t)B * D * 4); T_PTR(dimg);
      rc = compact ? HK().memo_gather(ginp.p<int>(), glist.p<int>(), n, T, gen_idx, n_mask, mask_id, record ? gkey.p<int>() : nullptr,
                                      ginpc.p<int>(), dimg, D, gimgc.p<float>(), nullptr)
                   : HK().memo_gather(ginp.p<int>(), nullptr, B, T, gen_idx, n_mask, mask_id, record ? gkey.p<int>() : nullptr, nullptr, nullptr,
                                      D, nullptr, nullptr);
      std::vector<int> rows_c((size_t)m * T), max_c((size_t)m);
      std::vector<float> cos_c((size_t)m);
      for (int i = 0; i < m; ++i) {
        const int b = compact ? hl[i] : i;
        memcpy(&rows_c[(size_t)i * T], new_rows + (size_t)b * T, (size_t)T * 4);
        cos_c[i] = new_cos[b]; max_c[i] = new_max[b];
      }
      int* drows = (int*)pool.up(rows_c.data(), rows_c.size() * 4); T_PTR(drows);
      float* dcos = (float*)pool.up(cos_c.data(), cos_c.size() * 4); T_PTR(dcos);
      int* dmax = (int*)pool.up(max_c.data(), max_c.size() * 4); T_PTR(dmax);
      if (rc == 0)
        rc = HK().memo_scatter(drows, dcos, dmax, compact ? glist.p<int>() : nullptr, m, T, ginp.p<int>(), gbcos.p<float>(),
                               record ? grows.p<int>() : nullptr, record ? gcos.p<float>() : nullptr, record ? gmax.p<int>() : nullptr, nullptr);
    }
    T_HIP(hipDeviceSynchronize());
  }
  T_CHECK(ghit.down(hit)); T_CHECK(glist.down(list)); T_CHECK(gtot.down(tot)); T_CHECK(gkey.down(key_out)); T_CHECK(ginp.down(inp_out));
  T_CHECK(gbcos.down(bcos_out)); T_CHECK(grows.down(ent_rows_out)); T_CHECK(gcos.down(ent_cos_out)); T_CHECK(gmax.down(ent_max_out));
  T_CHECK(ginpc.down(inp_c)); T_CHECK(gimgc.down(img_c));
  return launch_status(rc);
}

// The rows memo of czc_generate_rows, sub-step j of a group, as engine.hip chains it: launch_memo_rows_check; then (stages != 0), with n
// = tot[0]: launch_memo_rows_fill when n < R; nothing more when n == 0; else launch_memo_rows_gather (use_list: compact batch of the
// listed rows; else all R rows in place, recording only), "the step" (new_rows / new_cos / new_max of each row), launch_memo_rows_scatter.
// Table in / out (guarded): valid, sig [L*R], key [L*R*T], rows [L*2*R*T], cos, imax [L*2*R].  tau NULL or [R]: czc_draw taus.
// col / dot [R]: this step's schedule slice.  Out: hit [R], cnt [(R + 255) / 256], list [R], tot [4], inp_out [R*T], bcos_out [R], inp_c
// [R*T], img_c [R*D], col_c, dot_c [R].
int czc_test_memo_rows_chain(int R, int T, int L, int seed_len, int D, int n_mask0, int n_sub, int mask_id, int j, int stages, int use_list,
                             int record, const int32_t* inp, const int32_t* col0, const int32_t* col1, const float* tau, const int32_t* col,
                             const int32_t* dot, const float* img_n, const int32_t* new_rows, const float* new_cos, const int32_t* new_max,
                             const float* bcos_in, const int32_t* valid, const int32_t* sig, const int32_t* key, const int32_t* rows,
                             const float* cos, const int32_t* imax, int32_t* valid_out, int32_t* sig_out, int32_t* key_out, int32_t* rows_out,
                             float* cos_out, int32_t* imax_out, int32_t* hit, int32_t* cnt, int32_t* list, int32_t* tot, int32_t* inp_out,
                             float* bcos_out, int32_t* inp_c, float* img_c, int32_t* col_c, int32_t* dot_c) {
  const char* who = "memo_rows_chain";
  T_ARG(R >= 1 && R <= CZC_MAX_ROWS && T >= 1 && L >= 1 && L <= 64 && seed_len >= 0 && D >= 1 && n_mask0 >= 0 && n_sub >= 1 && n_sub <= MEMO_ROWS_SUB &&
        j >= 0 && j < MEMO_ROWS_SUB, who);
  const size_t rt = (size_t)R * T, lr = (size_t)L * R, nb = (size_t)(R + 255) / 256;
  DevPool pool;
  Guarded ginp, gvalid, gsig, gkey, grows, gcos, gimax, ghit, gcnt, glist, gtot, gbcos, ginpc, gimgc, gcolc, gdotc;
  T_CHECK(guarded_in(pool, ginp, inp, rt)); T_CHECK(guarded_in(pool, gvalid, valid, lr)); T_CHECK(guarded_in(pool, gsig, sig, lr));
  T_CHECK(guarded_in(pool, gkey, key, lr * T)); T_CHECK(guarded_in(pool, grows, rows, lr * MEMO_ROWS_SUB * T));
  T_CHECK(guarded_in(pool, gcos, cos, lr * MEMO_ROWS_SUB)); T_CHECK(guarded_in(pool, gimax, imax, lr * MEMO_ROWS_SUB));
  T_CHECK(ghit.make(pool, R)); T_CHECK(gcnt.make(pool, nb)); T_CHECK(glist.make(pool, R)); T_CHECK(gtot.make(pool, 4));
  T_CHECK(guarded_in(pool, gbcos, bcos_in, R)); T_CHECK(ginpc.make(pool, rt)); T_CHECK(gimgc.make(pool, (size_t)R * D));
  T_CHECK(gcolc.make(pool, R)); T_CHECK(gdotc.make(pool, R));
  int* dcol0 = (int*)pool.up(col0, (size_t)R * 4); T_PTR(dcol0);
  int* dcol1 = col1 ? (int*)pool.up(col1, (size_t)R * 4) : nullptr;
  if (col1) T_PTR(dcol1);
  RowDraw* ddraw = nullptr;
  if (tau) {
    std::vector<RowDraw> hd((size_t)R, RowDraw{0u, 0u, 0.f, 0u});
    for (int r = 0; r < R; ++r) hd[r].tau = tau[r];
    ddraw = (RowDraw*)pool.up(hd.data(), hd.size() * sizeof(RowDraw)); T_PTR(ddraw);
  }
  MemoRowsTab m;
  m.valid = gvalid.p<int>(); m.sig = gsig.p<int>(); m.key = gkey.p<int>(); m.rows = grows.p<int>(); m.cos = gcos.p<float>();
  m.imax = gimax.p<int>(); m.R = R; m.T = T; m.L = L; m.seed_len = seed_len;
  int rc = HK().memo_rows_check(ginp.p<int>(), m, dcol0, dcol1, n_mask0, n_sub, mask_id, ghit.p<int>(), gcnt.p<int>(), glist.p<int>(),
                                gtot.p<int>(), nullptr, ddraw);
  T_HIP(hipDeviceSynchronize());
  if (rc == 0 && stages) {
    int n = 0;
    T_HIP(hipMemcpy(&n, gtot.p<int>(), 4, hipMemcpyDeviceToHost));
    T_ARG(n >= 0 && n <= R, who);
    std::vector<int> hl((size_t)R);
    T_HIP(hipMemcpy(hl.data(), glist.p<int>(), (size_t)R * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) T_ARG(hl[i] >= 0 && hl[i] < R, who);
    if (n < R) rc = HK().memo_rows_fill(ghit.p<int>(), m, dcol0, j, ginp.p<int>(), gbcos.p<float>(), nullptr);
    if (rc == 0 && n > 0) {
      const bool compact = use_list != 0;
      const int cnt_rows = compact ? n : R;
      int* dcol = (int*)pool.up(col, (size_t)R * 4); T_PTR(dcol);
      int* ddot = (int*)pool.up(dot, (size_t)R * 4); T_PTR(ddot);
      float* dimg = (float*)pool.up(img_n, (size_t)R * D * 4); T_PTR(dimg);
      rc = compact ? HK().memo_rows_gather(ginp.p<int>(), glist.p<int>(), n, m, dcol0, dcol1, n_mask0, n_sub, mask_id, record ? 1 : 0, dcol, ddot,
                                           ginpc.p<int>(), dimg, D, gimgc.p<float>(), gcolc.p<int>(), gdotc.p<int>(), nullptr)
                   : (record ? HK().memo_rows_gather(ginp.p<int>(), nullptr, R, m, dcol0, dcol1, n_mask0, n_sub, mask_id, 1, dcol, ddot, nullptr,
                                                     nullptr, D, nullptr, nullptr, nullptr, nullptr)
                             : 0);
      std::vector<int> rows_c((size_t)cnt_rows * T), max_c((size_t)cnt_rows);
      std::vector<float> cos_c((size_t)cnt_rows);
      for (int i = 0; i < cnt_rows; ++i) {
        const int r = compact ? hl[i] : i;
        memcpy(&rows_c[(size_t)i * T], new_rows + (size_t)r * T, (size_t)T * 4);
        cos_c[i] = new_cos[r]; max_c[i] = new_max[r];
      }
      int* drows = (int*)pool.up(rows_c.data(), rows_c.size() * 4); T_PTR(drows);
      float* dcos = (float*)pool.up(cos_c.data(), cos_c.size() * 4); T_PTR(dcos);
      int* dmax = (int*)pool.up(max_c.data(), max_c.size() * 4); T_PTR(dmax);
      if (rc == 0)
        rc = HK().memo_rows_scatter(drows, dcos, dmax, compact ? glist.p<int>() : nullptr, cnt_rows, m, dcol0, j, record ? 1 : 0, ginp.p<int>(),
                                    gbcos.p<float>(), nullptr);
    }
    T_HIP(hipDeviceSynchronize());
  }
  T_CHECK(gvalid.down(valid_out)); T_CHECK(gsig.down(sig_out)); T_CHECK(gkey.down(key_out)); T_CHECK(grows.down(rows_out));
  T_CHECK(gcos.down(cos_out)); T_CHECK(gimax.down(imax_out)); T_CHECK(ghit.down(hit)); T_CHECK(gcnt.down(cnt)); T_CHECK(glist.down(list));
  T_CHECK(gtot.down(tot)); T_CHECK(ginp.down(inp_out)); T_CHECK(gbcos.down(bcos_out)); T_CHECK(ginpc.down(inp_c)); T_CHECK(gimgc.down(img_c));
  T_CHECK(gcolc.down(col_c)); T_CHECK(gdotc.down(dot_c));
  return launch_status(rc);
}

// ---- caption fluency (fluency.hip) ------------------------------------------------------------------------------------------
int czc_test_logprob(int N, int V, const float* logits, const int32_t* target, float temperature, float* logp, int32_t* rank,
                     int32_t* nonfinite) {
  const char* who = "logprob";
  T_ARG(N >= 1 && V >= 1 && (long)N * V < (1l << 28) && logits && target && logp && rank && nonfinite && all_in(target, N, 0, V), who);
  DevPool pool;
  float* dl = (float*)pool.up(logits, (size_t)N * V * 4); T_PTR(dl);
  int* dt = (int*)pool.up(target, (size_t)N * 4); T_PTR(dt);
  float* dp = (float*)pool.alloc((size_t)N * 4); T_PTR(dp);
  int* dr = (int*)pool.alloc((size_t)N * 4); T_PTR(dr);
  int* df = (int*)pool.alloc(4); T_PTR(df);
  T_HIP(hipMemset(df, 0, 4));
  const int rc = HK().logprob_target(dl, N, V, dt, temperature, nullptr, dp, dr, df, nullptr);
  T_HIP(hipDeviceSynchronize());
  if (rc) return launch_status(rc);
  T_HIP(hipMemcpy(logp, dp, (size_t)N * 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(rank, dr, (size_t)N * 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(nonfinite, df, 4, hipMemcpyDeviceToHost));
  return 0;
}

int czc_test_expand_mask(int R, int T, int seed_len, int mask_id, const int32_t* rows, const int32_t* len_of_row, int32_t* ids_out,
                         int32_t* target, int32_t* gen_rows, int32_t* n_seq) {
  const char* who = "expand_mask";
  T_ARG(R >= 1 && R <= (1 << 14) && T >= 1 && T <= 4096 && seed_len >= 0 && T - seed_len - 1 >= 1 && rows && ids_out && target && gen_rows && n_seq, who);
  const int Lmax = T - seed_len - 1;
  T_ARG(!len_of_row || all_in(len_of_row, R, 1, Lmax + 1), who);
  std::vector<int32_t> ros((size_t)R * Lmax), col((size_t)R * Lmax);
  const int N = HK().fluency_expand_tables(R, seed_len, Lmax, len_of_row, ros.data(), col.data());
  T_ARG(N >= 1 && N <= R * Lmax && all_in(ros.data(), N, 0, R) && all_in(col.data(), N, 0, T), who);  // what the kernel follows
  DevPool pool;
  int* drows = (int*)pool.up(rows, (size_t)R * T * 4); T_PTR(drows);
  int* dros = (int*)pool.up(ros.data(), (size_t)N * 4); T_PTR(dros);
  int* dcol = (int*)pool.up(col.data(), (size_t)N * 4); T_PTR(dcol);
  int* dids = (int*)pool.alloc((size_t)N * T * 4); T_PTR(dids);
  int* dtgt = (int*)pool.alloc((size_t)N * 4); T_PTR(dtgt);
  int* dgen = (int*)pool.alloc((size_t)N * 4); T_PTR(dgen);
  T_HIP(hipMemset(dids, 0x5a, (size_t)N * T * 4));
  T_HIP(hipMemset(dtgt, 0x5a, (size_t)N * 4));
  T_HIP(hipMemset(dgen, 0x5a, (size_t)N * 4));
  const int rc = HK().expand_mask_rows(drows, T, dros, dcol, N, mask_id, dids, dtgt, dgen, nullptr);
  T_HIP(hipDeviceSynchronize());
  if (rc) return launch_status(rc);
  T_HIP(hipMemcpy(ids_out, dids, (size_t)N * T * 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(target, dtgt, (size_t)N * 4, hipMemcpyDeviceToHost));
  T_HIP(hipMemcpy(gen_rows, dgen, (size_t)N * 4, hipMemcpyDeviceToHost));
  *n_seq = N;
  return 0;
}

// ---- the text bridge with candidates, the per-row forms of the top-K selection (bridge.hip, topk.hip) ---------------------------
int czc_test_bridge_cand(const czc_bridge_tables* t, int form, int B, int T, int K, const int32_t* inp, int gen_idx, const int32_t* gen_rows,
                         const int32_t* row_len, const int32_t* cand, const float* lexicon, const float* lex_pos, const uint8_t* lex_cls,
                         const uint8_t* tag_of_token, const uint16_t* masks, int n_masks, int negative, const czc_hyper* hp_rows,
                         int32_t* clip_ids, int32_t* clip_len, float* senti_raw, float* repeats, int32_t* overflow) {
  const char* who = "bridge_cand";
  T_ARG(t && form >= 0 && form <= 2 && B >= 1 && K >= 1 && (long)B * K <= (1 << 20) && T >= 1 && T <= CZC_MAX_BERT_LEN && inp, who);
  T_ARG(clip_ids && clip_len && senti_raw && repeats && overflow, who);
  const int V = t->bert_vocab;
  // every index the kernel follows, checked here: nothing out of bounds reaches the launch
  T_ARG(all_in(inp, (size_t)B * T, 0, V) && (!cand || all_in(cand, (size_t)B * K, 0, V)), who);
  T_ARG(cand || form != 0 || K == 1, who);  // verbatim rows (launch_bridge without candidates); the per-row launchers refuse a null cand themselves
  T_ARG(form == 0 ? (!cand || (gen_idx >= 0 && gen_idx < T)) : (!gen_rows || all_in(gen_rows, B, 0, T)), who);
  T_ARG(!row_len || all_in(row_len, B, 1, T + 1), who);
  T_ARG(!lex_pos == !lex_cls && (!lex_cls || [&] { for (int i = 0; i < V; ++i) if (lex_cls[i] >= 5) return false; return true; }()), who);
  T_ARG(!tag_of_token == !masks && (!masks || n_masks >= 1), who);
  T_ARG(!tag_of_token || [&] { for (int i = 0; i < V; ++i) if (tag_of_token[i] >= 15) return false; return true; }(), who);
  static_assert(sizeof(RowHyper) == sizeof(czc_hyper), "RowHyper is czc_hyper as the kernels read it");
  DevPool pool;
  BridgeDev bd;
  T_CHECK(bridge_tables_dev(pool, t, bd));
  const size_t bk = (size_t)B * K;
  int* dinp = (int*)pool.up(inp, (size_t)B * T * 4); T_PTR(dinp);
  int *dgen = nullptr, *dlen = nullptr, *dcand = nullptr;
  float *dlex = nullptr, *dlp = nullptr;
  uint8_t *dlc = nullptr, *dtag = nullptr;
  uint16_t* dmask = nullptr;
  RowHyper* dhp = nullptr;
  if (gen_rows) { dgen = (int*)pool.up(gen_rows, (size_t)B * 4); T_PTR(dgen); }
  if (row_len) { dlen = (int*)pool.up(row_len, (size_t)B * 4); T_PTR(dlen); }
  if (cand) { dcand = (int*)pool.up(cand, bk * 4); T_PTR(dcand); }
  if (lexicon) { dlex = (float*)pool.up(lexicon, (size_t)V * 4); T_PTR(dlex); }
  if (lex_pos) { dlp = (float*)pool.up(lex_pos, (size_t)V * 5 * 4); T_PTR(dlp); dlc = (uint8_t*)pool.up(lex_cls, (size_t)V); T_PTR(dlc); }
  if (tag_of_token) {
    dtag = (uint8_t*)pool.up(tag_of_token, (size_t)V); T_PTR(dtag);
    dmask = (uint16_t*)pool.up(masks, (size_t)n_masks * 2); T_PTR(dmask);
  }
  if (hp_rows) { dhp = (RowHyper*)pool.up(hp_rows, (size_t)B * sizeof(czc_hyper)); T_PTR(dhp); }
  Guarded gids, glen, gs, gr, govf;
  T_CHECK(gids.make(pool, bk * CZC_CLIP_MAX_LEN)); T_CHECK(glen.make(pool, bk)); T_CHECK(gs.make(pool, bk)); T_CHECK(gr.make(pool, bk));
  T_CHECK(govf.make(pool, 1)); T_CHECK(govf.zero(1));
  const PosDev pos{dtag, dmask, dtag ? n_masks : 0};
  int rc;
  if (form == 0)
    rc = launch_bridge(bd, dinp, B, T, cand ? gen_idx : -1, dcand, K, dlex, dlp, dlc, negative, pos, gids.p<int>(), glen.p<int>(), gs.p<float>(),
                       gr.p<float>(), govf.p<int>(), nullptr);
  else if (form == 1)
    rc = HK().bridge_rows(bd, dinp, B, T, dgen, dcand, K, dlex, dlp, dlc, negative, pos, gids.p<int>(), glen.p<int>(), gs.p<float>(),
                          gr.p<float>(), govf.p<int>(), nullptr, dlen);
  else
    rc = HK().bridge_rows_hp(bd, dinp, B, T, dgen, dcand, K, dlex, dlp, dlc, dhp, pos, gids.p<int>(), glen.p<int>(), gs.p<float>(),
                             gr.p<float>(), govf.p<int>(), nullptr, dlen);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gids.down(clip_ids)); T_CHECK(glen.down(clip_len)); T_CHECK(gs.down(senti_raw)); T_CHECK(gr.down(repeats));
  T_CHECK(govf.down(overflow));
  return launch_status(rc);
}

int czc_test_topk_rows(int form, int B, int V, int K, const float* logits, const float* mask, float temperature, int dot_id,
                       const int32_t* dot_rows, const czc_hyper* hp_rows, float* probs, int32_t* idxs, int32_t* cand) {
  const char* who = "topk_rows";
  T_ARG((form == 1 || form == 2) && B >= 1 && B <= (1 << 14) && V >= 1 && K >= 1 && logits && mask && probs && idxs && cand, who);
  T_ARG(form == 2 || (dot_rows && temperature > 0.f), who);  // only the hyper-parameter form checks its own pointers
  DevPool pool;
  float* dl = (float*)pool.up(logits, (size_t)B * V * 4); T_PTR(dl);
  float* dm = (float*)pool.up(mask, (size_t)V * 4); T_PTR(dm);
  int* dd = nullptr;
  RowHyper* dhp = nullptr;
  if (dot_rows) { dd = (int*)pool.up(dot_rows, (size_t)B * 4); T_PTR(dd); }
  if (hp_rows) { dhp = (RowHyper*)pool.up(hp_rows, (size_t)B * sizeof(czc_hyper)); T_PTR(dhp); }
  Guarded gp, gi, gc;
  const size_t bk = (size_t)B * K;
  T_CHECK(gp.make(pool, bk)); T_CHECK(gi.make(pool, bk)); T_CHECK(gc.make(pool, bk));
  const int rc = form == 1 ? HK().softmax_mask_topk_rows(dl, B, V, K, dm, temperature, dot_id, dd, gp.p<float>(), gi.p<int>(), gc.p<int>(), nullptr)
                           : HK().softmax_mask_topk_rows_hp(dl, B, V, K, dm, dhp, dot_id, dd, gp.p<float>(), gi.p<int>(), gc.p<int>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gp.down(probs)); T_CHECK(gi.down(idxs)); T_CHECK(gc.down(cand));
  return launch_status(rc);
}

int czc_test_topk_rows_vocab(int B, int V, int K, const float* logits, const float* mask, int dot_id, const int32_t* dot_rows,
                             const czc_hyper* hp_rows, const int32_t* set_rows, const uint32_t* bits, int n_sets, int W, float* probs,
                             int32_t* idxs, int32_t* cand) {
  const char* who = "topk_rows_vocab";
  T_ARG(B >= 1 && B <= (1 << 14) && V >= 1 && K >= 1 && logits && mask && probs && idxs && cand, who);
  T_ARG(n_sets >= 0 && n_sets <= (1 << 12) && W >= 0 && W <= (1 << 16), who);
  // every index the kernel follows, checked here: nothing out of bounds reaches the launch (the launcher checks W against V, and
  // refuses a null pointer before anything is read)
  T_ARG(!set_rows || !bits || all_in(set_rows, B, -1, n_sets), who);
  T_ARG(!bits || (n_sets >= 1 && W >= 1), who);
  DevPool pool;
  float* dl = (float*)pool.up(logits, (size_t)B * V * 4); T_PTR(dl);
  float* dm = (float*)pool.up(mask, (size_t)V * 4); T_PTR(dm);
  int *dd = nullptr, *ds = nullptr;
  unsigned* db = nullptr;
  RowHyper* dhp = nullptr;
  if (dot_rows) { dd = (int*)pool.up(dot_rows, (size_t)B * 4); T_PTR(dd); }
  if (hp_rows) { dhp = (RowHyper*)pool.up(hp_rows, (size_t)B * sizeof(czc_hyper)); T_PTR(dhp); }
  if (set_rows) { ds = (int*)pool.up(set_rows, (size_t)B * 4); T_PTR(ds); }
  if (bits) { db = (unsigned*)pool.up(bits, (size_t)n_sets * W * 4); T_PTR(db); }
  Guarded gp, gi, gc;
  const size_t bk = (size_t)B * K;
  T_CHECK(gp.make(pool, bk)); T_CHECK(gi.make(pool, bk)); T_CHECK(gc.make(pool, bk));
  const int rc = HK().softmax_mask_topk_rows_vocab(dl, B, V, K, dm, dhp, dot_id, dd, ds, db, W, gp.p<float>(), gi.p<int>(), gc.p<int>(), nullptr);
  T_HIP(hipDeviceSynchronize());
  T_CHECK(gp.down(probs)); T_CHECK(gi.down(idxs)); T_CHECK(gc.down(cand));
  return launch_status(rc);
}

}  // extern "C"

// ---- czc_test_gemm_layout: one GEMM launch on strided, windowed and in-place buffers ----------------------------------------
namespace {

// A 2-D buffer of the layout hook: `rows` rows of `ld` elements of `es` bytes, CZC_TEST_LAYOUT_GUARD rows in front of them and
// `back` rows behind them (to the end of the last 256-row tile and CZC_TEST_LAYOUT_GUARD more), every 32-bit word pre-filled.
struct Padded {
  unsigned char* base = nullptr;
  size_t rows = 0, back = 0, ld = 0, es = 0;
  size_t bytes() const { return (CZC_TEST_LAYOUT_GUARD + rows + back) * ld * es; }
  unsigned char* at(size_t c0) const { return base + ((size_t)CZC_TEST_LAYOUT_GUARD * ld + c0) * es; }
  int make(DevPool& pool, size_t rows_, size_t ld_, size_t es_, uint32_t fill) {
    rows = rows_; ld = ld_; es = es_;
    back = (256 - rows % 256) % 256 + CZC_TEST_LAYOUT_GUARD;
    const size_t words = (bytes() + 3) / 4;
    base = (unsigned char*)pool.alloc(words * 4); T_PTR(base);
    T_HIP(hipMemsetD32((hipDeviceptr_t)base, (int)fill, words));
    return 0;
  }
  // a dense [rows, width] device array of the same element type -> columns c0 .. c0 + width of the rows
  int put(const void* dense, size_t width, size_t c0) const {
    T_HIP(hipMemcpy2D(at(c0), ld * es, dense, width * es, width * es, rows, hipMemcpyDeviceToDevice));
    return 0;
  }
  int down(void* host) const {
    T_HIP(hipMemcpy(host, base, bytes(), hipMemcpyDeviceToHost));
    return 0;
  }
};

// quiet NaNs of an element type, as 32-bit words (fp16 planes for the split type)
uint32_t nan_words(int prec) { return prec == PREC_F32 ? 0x7fc00000u : prec == PREC_BF16 ? 0x7fc07fc0u : 0x7e007e00u; }
constexpr uint32_t SENTINEL_WORDS = 0x5a5a5a5au;

// 0, CZC_TEST_REFUSED (the launcher refused: nothing ran) or a CZC_ERR_* status; *family = what the launcher recorded
int gemm_layout_run(const czc_gemm_layout* c, int* family) {
  const char* who = "gemm_layout";
  const int P = c->precision, M = c->M, N = c->N, K = c->K, form = c->form;
  const bool half = P == PREC_BF16 || P == PREC_F16;
  const bool in_place = c->flags & CZC_GEMM_IN_PLACE, both = c->flags & CZC_GEMM_BOTH_OUTPUTS, typed = c->flags & CZC_GEMM_TYPED_OUT;
  T_ARG(half || P == PREC_F32 || P == PREC_F16X3, who);
  T_ARG(form >= CZC_GEMM_FORM_PLAIN && form <= CZC_GEMM_FORM_ROWLN && (form == CZC_GEMM_FORM_PLAIN || half), who);
  T_ARG(M >= 1 && N >= 1 && K >= 1 && M <= (1 << 20) && N <= (1 << 16) && K <= (1 << 16) && c->A && c->W, who);
  T_ARG(c->lda >= K && c->ldw >= K && c->c0 >= 0 && c->ldc >= c->c0 + N && c->lda <= 2 * K + 64 && c->ldw <= 2 * K + 64 && c->ldc <= 4 * N + 64, who);
  T_ARG(!c->resid || (c->ldr >= c->c0 + N && c->ldr <= 4 * N + 64), who);
  T_ARG(!in_place || (c->resid && c->ldr == c->ldc), who);
  T_ARG(P != PREC_F16X3 || (K % 8 == 0 && c->lda % 8 == 0 && c->ldw % 8 == 0), who);  // whole hi / lo groups per row
  const bool want_f32 = form == CZC_GEMM_FORM_X16 || form == CZC_GEMM_FORM_ROWLN || (form == CZC_GEMM_FORM_PLAIN && (!typed || both));
  const bool want_act = form == CZC_GEMM_FORM_LNF || form == CZC_GEMM_FORM_ROWLN || (form == CZC_GEMM_FORM_PLAIN && (typed || both));
  T_ARG((!want_f32 || c->out_f32) && (!want_act || c->out_act) && !(typed && both), who);
  T_ARG(!in_place || want_f32, who);
  T_ARG(P != PREC_F16X3 || !want_act || (c->ldc % 8 == 0 && c->c0 % 8 == 0), who);  // split_t rows: groups of 8 from the buffer's start
  if (form == CZC_GEMM_FORM_X16) T_ARG(c->resid && K % 8 == 0 && (c->part_ld == 0 || (c->part_ld >= M && N % 32 == 0 && c->part_out)), who);
  else T_ARG(c->part_ld == 0, who);
  if (form == CZC_GEMM_FORM_LNF) T_ARG(K == 512 && c->bias && c->gamma && c->beta && c->ln_part && !c->resid, who);
  if (form == CZC_GEMM_FORM_ROWLN) T_ARG(N == 512 && c->resid && c->gamma && c->beta, who);

  DevPool pool;
  const int a_prec = form == CZC_GEMM_FORM_LNF ? PREC_F16 : P;  // lnf: A is the raw fp16 residual stream
  const size_t es = prec_bytes(P);
  // operands: NaN pads and guards
  Padded pA, pW, pR;
  T_CHECK(pA.make(pool, M, c->lda, prec_bytes(a_prec), nan_words(a_prec)));
  {
    void* d = up_act(pool, a_prec, c->A, (size_t)M * K); T_PTR(d);
    T_CHECK(pA.put(d, K, 0));
  }
  float* dB = nullptr;  // N entries, then a NaN tail the kernel must not read
  auto up_bias = [&](const float* dev_or_host, hipMemcpyKind kind) -> int {
    dB = (float*)pool.alloc((size_t)(N + 64) * 4); T_PTR(dB);
    T_HIP(hipMemsetD32((hipDeviceptr_t)dB, (int)nan_words(PREC_F32), (size_t)N + 64));
    T_HIP(hipMemcpy(dB, dev_or_host, (size_t)N * 4, kind));
    return 0;
  };
  float* dstat = nullptr;
  float* dpart_in = nullptr;
  bool stats_in_kernel = false;
  if (form == CZC_GEMM_FORM_LNF) {  // the preparation of czc_test_ln_fold_gemm, the folded weights then placed at ldw
    T_CHECK(pW.make(pool, N, c->ldw, 2, nan_words(PREC_F16)));
    float* dW = (float*)pool.up(c->W, (size_t)N * K * 4); T_PTR(dW);
    float* dg = (float*)pool.up(c->gamma, (size_t)K * 4); T_PTR(dg);
    float* dbt = (float*)pool.up(c->beta, (size_t)K * 4); T_PTR(dbt);
    float* db = (float*)pool.up(c->bias, (size_t)N * 4); T_PTR(db);
    dpart_in = (float*)pool.up(c->ln_part, (size_t)16 * M * 8); T_PTR(dpart_in);
    dstat = (float*)pool.alloc((size_t)M * 8 + 256); T_PTR(dstat);
    void* dWf = pool.alloc((size_t)N * K * 2); T_PTR(dWf);
    float* dcs = (float*)pool.alloc((size_t)N * 4); T_PTR(dcs);
    float* dbf = (float*)pool.alloc((size_t)N * 4); T_PTR(dbf);
    stats_in_kernel = gemm_wreg_stats_in_kernel(M, N);
    if (!stats_in_kernel) T_CHECK(launch_ln_finalize(dpart_in, M, 16, M, c->eps, dstat, nullptr));
    T_CHECK(launch_fold_ln(dW, dg, dbt, db, N, K, dWf, dcs, dbf, nullptr));
    T_HIP(hipDeviceSynchronize());
    T_CHECK(pW.put(dWf, K, 0));
    T_CHECK(up_bias(dbf, hipMemcpyDeviceToDevice));
  } else {
    T_CHECK(pW.make(pool, N, c->ldw, es, nan_words(P)));
    void* d = up_act(pool, P, c->W, (size_t)N * K); T_PTR(d);
    T_CHECK(pW.put(d, K, 0));
    if (c->bias) T_CHECK(up_bias(c->bias, hipMemcpyHostToDevice));
  }
  // outputs: the 0x5a pattern everywhere; out_f32 holds fp16 rows in the x16 form
  const size_t es_f = form == CZC_GEMM_FORM_X16 ? 2 : 4;
  const int r_prec = form == CZC_GEMM_FORM_X16 ? PREC_F16 : PREC_F32;
  Padded pF, pO;
  if (want_f32) T_CHECK(pF.make(pool, M, c->ldc, es_f, SENTINEL_WORDS));
  if (want_act) T_CHECK(pO.make(pool, M, c->ldc, es, SENTINEL_WORDS));
  const void* resid_p = nullptr;
  if (c->resid) {
    void* d = up_act(pool, r_prec, c->resid, (size_t)M * N); T_PTR(d);
    if (in_place) {
      T_CHECK(pF.put(d, N, c->c0));
      resid_p = pF.at(c->c0);
    } else {
      T_CHECK(pR.make(pool, M, c->ldr, es_f, nan_words(r_prec)));
      T_CHECK(pR.put(d, N, c->c0));
      resid_p = pR.at(c->c0);
    }
  }
  Guarded gpart;
  if (c->part_ld) T_CHECK(gpart.make(pool, (size_t)(N / 32) * c->part_ld * 2));
  T_HIP(hipDeviceSynchronize());

  GemmArgs g;
  g.A = pA.at(0); g.lda = c->lda; g.W = pW.at(0); g.ldw = c->ldw; g.bias = dB;
  g.resid = (const float*)resid_p; g.ldr = c->resid ? c->ldr : 0;
  g.out_f32 = want_f32 ? (float*)pF.at(c->c0) : nullptr;
  g.out_act = want_act ? (void*)pO.at(c->c0) : nullptr;
  g.ldc = c->ldc; g.M = M; g.N = N; g.K = K; g.act = c->act;
  int rc;
  if (form == CZC_GEMM_FORM_ROWLN) {
    float* dg = (float*)pool.up(c->gamma, (size_t)N * 4); T_PTR(dg);
    float* dbt = (float*)pool.up(c->beta, (size_t)N * 4); T_PTR(dbt);
    g.ln_gamma = dg; g.ln_beta = dbt; g.ln_eps = c->eps; g.f16 = P == PREC_F16;
    rc = launch_gemm_rowln(g, nullptr);
  } else {
    if (form == CZC_GEMM_FORM_X16) {
      g.x16 = 1;
      if (c->part_ld) { g.row_part = gpart.p<float>(); g.part_ld = c->part_ld; }
    }
    if (form == CZC_GEMM_FORM_LNF) {
      g.ln_stat = dstat;
      if (stats_in_kernel) { g.ln_part = dpart_in; g.ln_part_ld = M; g.ln_eps = c->eps; }
    }
    rc = launch_gemm(P, g, nullptr);
  }
  *family = HK().gemm_family();
  if (rc > 1) return CZC_ERR_HIP;
  T_HIP(hipDeviceSynchronize());
  if (want_f32) T_CHECK(pF.down(c->out_f32));
  if (want_act) T_CHECK(pO.down(c->out_act));
  if (c->part_ld) T_CHECK(gpart.down(c->part_out));
  return rc == 1 ? CZC_TEST_REFUSED : 0;
}

}  // namespace

extern "C" {

int czc_test_gemm_family(void) { return HK().gemm_family(); }

int czc_test_gemm_layout(const czc_gemm_layout* c) {
  if (!c) { snprintf(TEST_ERR, 512, "gemm_layout: null argument"); return -CZC_ERR_ARG; }
  int family = 0;
  const int rc = gemm_layout_run(c, &family);
  if (rc == CZC_TEST_REFUSED) return 0;
  if (rc) return -rc;
  if (family <= 0) { snprintf(TEST_ERR, 512, "gemm_layout: the launcher recorded no family"); return -CZC_ERR_STATE; }
  return family;
}

// ---- the combine kernel in every instantiation without rivals (tests/test_combine_kernel_gpu.py against tests/combine_ref.py) ------
// form 0 <false,false,false> (gen_idx), 1 <true,false,false> (gen_rows), 2 <true,true,false> (+ hp_rows), 3 <true,true,true>
// (+ draw_rows).  The cosines come from text_feat / img_embeds (normalised by launch_l2_normalize) or, with text_feat null, from
// cos_in placed in clip_ref before the launch.  run [B] given: hp / draw hold R full records and the B compact rows' records are
// gathered on the device by launch_gather_row_hyper / launch_gather_row_draw (and returned in hp_out / draw_out).  Every output is
// Guarded; every index the kernels follow is checked here first.
int czc_test_combine_rows(int B, int K, int D, int T, const float* text_feat, const float* img_embeds, const float* cos_in,
                          float logit_scale, const float* probs, const int32_t* cand, const float* senti_raw, const float* repeats,
                          int form, const czc_hyper* hp, const czc_draw* draw, uint32_t draw_step, int gen_idx, const int32_t* gen_rows,
                          const int32_t* run, int R, const int32_t* inp_in, int32_t* inp_out, float* clip_score, float* clip_ref,
                          float* final_score, int32_t* best, float* best_cos, int32_t* nonfinite, int32_t* hp_out, int32_t* draw_out,
                          float* scale_out) {
  const char* who = "combine_rows";
  static_assert(sizeof(RowHyper) == sizeof(czc_hyper) && sizeof(RowHyper) == 24, "RowHyper is czc_hyper as the kernels read it");
  static_assert(sizeof(RowDraw) == sizeof(czc_draw) && sizeof(RowDraw) == 16, "RowDraw is czc_draw as the kernels read it");
  T_ARG(B >= 1 && K >= 1 && form >= 0 && form <= 3 && (long)B * K <= (1 << 22), who);
  T_ARG((text_feat != nullptr) != (cos_in != nullptr), who);
  T_ARG(!text_feat || (img_embeds && D >= 1), who);
  T_ARG(probs && cand && hp && clip_score && clip_ref && final_score && best && best_cos && nonfinite, who);
  T_ARG((form == 3) == (draw != nullptr), who);
  T_ARG((inp_in != nullptr) == (inp_out != nullptr), who);
  T_ARG(!run || (form >= 2 && R >= 1 && all_in(run, B, 0, R) && hp_out && (form < 3 || draw_out)), who);
  if (inp_in) {  // the write-back column of every row
    T_ARG(T >= 1, who);
    if (form == 0) T_ARG(gen_idx >= 0 && gen_idx < T, who);
    else T_ARG(gen_rows && all_in(gen_rows, B, 0, T), who);
  }
  for (int b = 0; b < (form >= 2 ? B : 1); ++b) {  // what a row's control signal makes the kernel read
    const czc_hyper& h = hp[run ? run[b] : b];
    T_ARG(h.control >= 0 && h.control <= 2, who);
    T_ARG(h.control != 1 || (senti_raw && repeats), who);
    T_ARG(h.control != 2 || senti_raw, who);
  }
  DevPool pool;
  const size_t bk = (size_t)B * K;
  float *dt = nullptr, *din = nullptr;
  if (text_feat) {
    dt = (float*)pool.up(text_feat, bk * D * 4); T_PTR(dt);
    float* di = (float*)pool.up(img_embeds, (size_t)B * D * 4); T_PTR(di);
    din = (float*)pool.alloc((size_t)B * D * 4); T_PTR(din);
    T_CHECK(launch_l2_normalize(di, B, D, din, nullptr));
  }
  float* dp = (float*)pool.up(probs, bk * 4); T_PTR(dp);
  int* dcand = (int*)pool.up(cand, bk * 4); T_PTR(dcand);
  float* ds = nullptr; float* dr = nullptr;
  if (senti_raw) { ds = (float*)pool.up(senti_raw, bk * 4); T_PTR(ds); }
  if (repeats) { dr = (float*)pool.up(repeats, bk * 4); T_PTR(dr); }
  int* dcol = nullptr;
  if (form >= 1) {
    dcol = (int*)pool.alloc((size_t)B * 4); T_PTR(dcol);
    if (gen_rows) T_HIP(hipMemcpy(dcol, gen_rows, (size_t)B * 4, hipMemcpyHostToDevice));
    else T_HIP(hipMemset(dcol, 0, (size_t)B * 4));  // nothing is written back
  }
  Guarded o1, o2, o3, ob, oc, gnf, ginp, ghp, gdr;
  T_CHECK(o1.make(pool, bk)); T_CHECK(o2.make(pool, bk)); T_CHECK(o3.make(pool, bk)); T_CHECK(ob.make(pool, B)); T_CHECK(oc.make(pool, B));
  T_CHECK(gnf.make(pool, 8));
  T_CHECK(gnf.zero(8));
  if (cos_in) T_CHECK(o2.fill(cos_in));
  if (inp_in) T_CHECK(guarded_in(pool, ginp, inp_in, (size_t)B * T));
  const RowHyper* dh = nullptr;
  const RowDraw* dd = nullptr;
  if (form >= 2) {
    const int n_rec = run ? R : B;
    RowHyper* full = (RowHyper*)pool.up(hp, (size_t)n_rec * sizeof(czc_hyper)); T_PTR(full);
    dh = full;
    RowDraw* dfull = nullptr;
    if (form == 3) { dfull = (RowDraw*)pool.up(draw, (size_t)n_rec * sizeof(czc_draw)); T_PTR(dfull); dd = dfull; }
    if (run) {
      int* drun = (int*)pool.up(run, (size_t)B * 4); T_PTR(drun);
      T_CHECK(ghp.make(pool, (size_t)B * 6));
      T_CHECK(launch_status(launch_gather_row_hyper(full, drun, B, ghp.p<RowHyper>(), nullptr)));
      dh = ghp.p<RowHyper>();
      if (form == 3) {
        T_CHECK(gdr.make(pool, (size_t)B * 4));
        T_CHECK(launch_status(launch_gather_row_draw(dfull, drun, B, gdr.p<RowDraw>(), nullptr)));
        dd = gdr.p<RowDraw>();
      }
    }
  }
  CombineArgs a;
  a.text_feat = dt; a.img_n = din; a.logit_scale_exp = expf(logit_scale); a.probs = dp; a.cand = dcand;
  a.senti_raw = ds; a.repeats = dr; a.alpha = hp->alpha; a.beta = hp->beta; a.gamma = hp->gamma; a.use_senti = hp->control;
  a.B = B; a.K = K; a.D = D; a.clip_score = o1.p<float>(); a.clip_ref = o2.p<float>(); a.final_score = o3.p<float>();
  a.best = ob.p<int>(); a.best_cos = oc.p<float>(); a.inp = inp_in ? ginp.p<int>() : nullptr; a.T = T; a.gen_idx = gen_idx;
  a.nonfinite = gnf.p<int>();
  a.gen_rows = dcol; a.hp_rows = dh; a.draw_rows = dd; a.draw_step = draw_step;
  if (scale_out) *scale_out = a.logit_scale_exp;  // the fp32 scale the kernel is given: an input of the kernel, exact to the reference
  const int rc = launch_combine(a, nullptr);
  T_HIP(hipDeviceSynchronize());
  if (rc > 1) return CZC_ERR_HIP;
  T_CHECK(o1.down(clip_score)); T_CHECK(o2.down(clip_ref)); T_CHECK(o3.down(final_score)); T_CHECK(ob.down(best)); T_CHECK(oc.down(best_cos));
  T_CHECK(gnf.down(nonfinite));
  if (inp_in) T_CHECK(ginp.down(inp_out));
  if (run) {
    T_CHECK(ghp.down(hp_out));
    if (form == 3) T_CHECK(gdr.down(draw_out));
  }
  return rc == 1 ? CZC_TEST_REFUSED : 0;
}

}  // extern "C"
