// Caption fluency (czc_fluency_rows): BERT's pseudo-log-likelihood of finished rows.
//
// R captions become N = sum L_r sequences, one per word, each the caption with that word masked (expand_mask_rows_kernel); BERT and
// the MLM head run on them as in a step; logprob_target_kernel turns every [V] logits row into log softmax(x / t) at the masked
// word's own id and that id's rank in the row; pll_sum_kernel adds a caption's log-probabilities up.
#include "kernels.h"

namespace czc {

// ---- host: which (row, column) every expanded sequence masks -------------------------------------------------------------
int fluency_expand_tables(int R, int seed_len, int Lmax, const int32_t* len_of_row, int32_t* row_of_seq, int32_t* col_of_seq) {
  int n = 0;
  for (int r = 0; r < R; ++r) {
    const int L = len_of_row ? len_of_row[r] : Lmax;
    for (int j = 0; j < L; ++j, ++n) {
      row_of_seq[n] = r;
      col_of_seq[n] = seed_len + j;
    }
  }
  return n;
}

// ---- expansion -----------------------------------------------------------------------------------------------------------
// thread (n, t): ids_out[n][t] = rows[row_of_seq[n]][t], the column col_of_seq[n] replaced by mask_id; the thread of that column
// also leaves the id it replaced and the column itself.  The columns behind a row's own tokens are copied as they stand.
__global__ __launch_bounds__(256) void expand_mask_rows_kernel(const int* rows, int T, const int* row_of_seq, const int* col_of_seq, int N,
                                                               int mask_id, int* ids_out, int* target, int* gen_rows) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * T) return;
  const int n = (int)(i / T), t = (int)(i % T);
  const int col = col_of_seq[n];
  const int id = rows[(long)row_of_seq[n] * T + t];
  if (t == col) {
    target[n] = id;
    gen_rows[n] = col;
    ids_out[i] = mask_id;
  } else {
    ids_out[i] = id;
  }
}

int launch_expand_mask_rows(const int* rows, int T, const int* row_of_seq, const int* col_of_seq, int N, int mask_id, int* ids_out,
                            int* target, int* gen_rows, hipStream_t st) {
  if (N <= 0) return 0;
  if (T <= 0 || !rows || !row_of_seq || !col_of_seq || !ids_out || !target || !gen_rows) {
    snprintf(g_err, sizeof(g_err), "expand_mask_rows: missing table or T=%d", T);
    return 1;
  }
  hipLaunchKernelGGL(expand_mask_rows_kernel, dim3(cdiv((long)N * T, 256)), dim3(256), 0, st, rows, T, row_of_seq, col_of_seq, N, mask_id,
                     ids_out, target, gen_rows);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- log-probability and rank at a target id --------------------------------------------------------------------------------
constexpr int LP_THREADS = 256;

// a lane's running (max, sum of exp(y - max)) and the two counts of the rank
struct LpAcc {
  float m = -INFINITY, s = 0.f;
  int gt = 0, eq = 0;
};

// up to four elements of the row starting at id i0 (cnt of them count)
__device__ __forceinline__ void lp_take(LpAcc& a, const float (&x)[4], int cnt, int i0, float temperature, float xt, int target) {
  float y[4];
  float mx = a.m;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    y[k] = x[k] / temperature;
    if (k < cnt) {
      mx = fmaxf(mx, y[k]);
      a.gt += x[k] > xt ? 1 : 0;
      a.eq += (x[k] == xt && i0 + k < target) ? 1 : 0;
    }
  }
  if (mx > a.m) {  // (a.m == -inf: s is 0 and stays 0)
    a.s = a.m == -INFINITY ? 0.f : a.s * expf(a.m - mx);
    a.m = mx;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < cnt) a.s += expf(y[k] - a.m);
}

// One work-group per sequence n, one pass over its row: logp[o] = (y_t - m) - logf(s) with y = x / temperature, m = max y,
// s = sum exp(y - m); rank[o] = #{i : x_i > x_t} + #{i < t : x_i == x_t} on the raw logits (ascending id among equals: the order
// of topk.hip).  o = out_idx ? out_idx[n] : n.  Every lane runs the online form over its share, then the lanes agree on the
// row maximum, rescale once and their sums go through a shuffle tree and 4 LDS words: no long serial chain.
// The row starts at byte n * V * 4: lanes peel single elements up to the first 16-byte boundary, then load float4, then the tail.
__global__ __launch_bounds__(LP_THREADS) void logprob_target_kernel(const float* logits, int V, const int* target, float temperature,
                                                                    const int* out_idx, float* logp, int* rank, int* nonfinite) {
  __shared__ float red_f[LP_THREADS / 64];
  __shared__ int red_i[2][LP_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x;
  const long o = out_idx ? out_idx[n] : n;
  const float* lr = logits + (long)n * V;
  const int t = target[n];
  if (t < 0 || t >= V) {  // (uniform over the work-group; the callers check their ids first)
    if (tid == 0) { logp[o] = NAN; rank[o] = -1; *nonfinite = 1; }
    return;
  }
  const float xt = lr[t];
  const int head = min(V, (int)(((16 - ((uintptr_t)lr & 15)) & 15) >> 2));
  const int nv = (V - head) >> 2, tail0 = head + 4 * nv;
  LpAcc a;
  if (tid < head) {
    const float x[4] = {lr[tid], 0.f, 0.f, 0.f};
    lp_take(a, x, 1, tid, temperature, xt, t);
  }
  const float4* body = (const float4*)(lr + head);
  for (int j = tid; j < nv; j += LP_THREADS) {
    const float4 v = body[j];
    const float x[4] = {v.x, v.y, v.z, v.w};
    lp_take(a, x, 4, head + 4 * j, temperature, xt, t);
  }
  if (tail0 + tid < V) {
    const float x[4] = {lr[tail0 + tid], 0.f, 0.f, 0.f};
    lp_take(a, x, 1, tail0 + tid, temperature, xt, t);
  }
  // the row maximum
  float m = wave_max(a.m);
  if (lane == 0) red_f[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red_f[0], red_f[1]), fmaxf(red_f[2], red_f[3]));
  __syncthreads();
  // the sum at that maximum, and the counts
  float s = wave_sum(a.m == -INFINITY ? 0.f : a.s * expf(a.m - m));
  int gt = a.gt, eq = a.eq;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    gt += __shfl_xor(gt, w, 64);
    eq += __shfl_xor(eq, w, 64);
  }
  if (lane == 0) { red_f[wave] = s; red_i[0][wave] = gt; red_i[1][wave] = eq; }
  __syncthreads();
  if (tid == 0) {
    s = (red_f[0] + red_f[1]) + (red_f[2] + red_f[3]);
    const float lp = (xt / temperature - m) - logf(s);
    logp[o] = lp;
    rank[o] = (red_i[0][0] + red_i[0][1]) + (red_i[0][2] + red_i[0][3]) + (red_i[1][0] + red_i[1][1]) + (red_i[1][2] + red_i[1][3]);
    if (!isfinite(lp)) *nonfinite = 1;
  }
}

int launch_logprob_target(const float* logits, int N, int V, const int* target, float temperature, const int* out_idx, float* logp,
                          int* rank, int* nonfinite, hipStream_t st) {
  if (N <= 0) return 0;
  if (V <= 0 || !(temperature > 0.f) || !logits || !target || !logp || !rank || !nonfinite) {
    snprintf(g_err, sizeof(g_err), "logprob_target: V=%d, temperature=%g or a missing buffer", V, (double)temperature);
    return 1;
  }
  hipLaunchKernelGGL(logprob_target_kernel, dim3(N), dim3(LP_THREADS), 0, st, logits, V, target, temperature, out_idx, logp, rank, nonfinite);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- pll[r] = logp[r][0] + ... + logp[r][len[r] - 1], in that order ---------------------------------------------------------
__global__ __launch_bounds__(256) void pll_sum_kernel(const float* logp, int R, int Lmax, const int* len_of_row, float* pll) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const int L = len_of_row ? min(len_of_row[r], Lmax) : Lmax;
  float s = 0.f;
  for (int j = 0; j < L; ++j) s += logp[(long)r * Lmax + j];
  pll[r] = s;
}

int launch_pll_sum(const float* logp, int R, int Lmax, const int* len_of_row, float* pll, hipStream_t st) {
  if (R <= 0) return 0;
  hipLaunchKernelGGL(pll_sum_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, logp, R, Lmax, len_of_row, pll);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace czc
