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
static int g_bridge_no_table = 0;  // czc_test_bridge: 1 = every chunk through the merge loop (option "bridge_no_table")  // czc_bench_gemm: extra elements per row of A and W (row pitch vs L2 channel experiments)

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
  unsigned char* d = (unsigned char*)pool.alloc((n + 2 * GR) * row); T_PTR(d);
  std::vector<uint32_t> nan((size_t)GR * row / 4, precision == PREC_BF16 ? 0x7fc07fc0u : 0x7e007e00u);
  T_HIP(hipMemcpy(d, nan.data(), (size_t)GR * row, hipMemcpyHostToDevice));
  T_HIP(hipMemcpy(d + (GR + n) * row, nan.data(), (size_t)GR * row, hipMemcpyHostToDevice));
  if (n) {
    float* f = (float*)pool.up(src, n * (row / 2) * 4); T_PTR(f);
    T_CHECK(launch_convert(precision, f, d + GR * row, (long)(n * (row / 2)), nullptr));
  }
  *rows0 = d + GR * row;
  return 0;
}
}  // namespace

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
