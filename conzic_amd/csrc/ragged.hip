// BERT on packed ragged rows (czc_generate_rows_len): sequence b of a batch has row_len[b] tokens, its rows sit at
// row_off[b] .. row_off[b] + row_len[b] - 1 of the packed [sum row_len, H] activations, and the ids it reads are the first
// row_len[b] columns of a row of the [*, T] strided id batch.  The padding columns behind them are never read.
// Same form as rowops.hip: one 64-lane wave per row, float4 accesses, shuffle reductions, fp32 statistics.
#include "kernels.h"

namespace czc {

// wave (b, t), t < max_T: token t of sequence b (a wave with t >= row_len[b] leaves at once).  The token takes position
// embedding t -- its place inside its own sequence -- and the arithmetic of bert_embed_kernel: HF's add order, ln_row.
template <typename T>
__global__ __launch_bounds__(256) void bert_embed_ragged_kernel(const int* ids, int ids_stride, const int* run, const int* row_off,
                                                                const int* row_len, int n, int max_T, int H, const float* word,
                                                                const float* pos, const float* type0, const float* gamma,
                                                                const float* beta, float eps, T* y_act, float* y_f32) {
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long)n * max_T) return;
  const int b = (int)(w / max_T), t = (int)(w % max_T);
  if (t >= row_len[b]) return;
  const long m = (long)row_off[b] + t;
  const int id = ids[(long)(run ? run[b] : b) * ids_stride + t];
  const float* wr = word + (long)id * H;
  const float* pr = pos + (long)t * H;
  float4 v[LN_MAXV];
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      const float4 a = *(const float4*)(wr + c), bb = *(const float4*)(type0 + c), d = *(const float4*)(pr + c);
      // HF order: inputs_embeds + token_type_embeddings, then + position_embeddings
      v[i] = make_float4((a.x + bb.x) + d.x, (a.y + bb.y) + d.y, (a.z + bb.z) + d.z, (a.w + bb.w) + d.w);
    } else {
      v[i] = make_float4(0, 0, 0, 0);
    }
  }
  ln_row<LN_MAXV>(v, H, lane, gamma, beta, eps);
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      if (y_f32) *(float4*)(y_f32 + m * H + c) = v[i];
      if (y_act) Act<T>::st4(y_act, m * H + c, v[i].x, v[i].y, v[i].z, v[i].w);
    }
  }
}

int launch_bert_embed_ragged(int prec, const int* ids, int ids_stride, const int* run, const int* row_off, const int* row_len, int n,
                             int max_T, int H, const float* word, const float* pos, const float* type0, const float* gamma,
                             const float* beta, float eps, void* y_act, float* y_f32, hipStream_t st) {
  if (n <= 0 || max_T <= 0) return 0;
  if (H <= 0 || H % 4 || H > LN_MAXV * 256 || (prec == PREC_F16X3 && y_act && H % 8) || max_T > ids_stride || !row_off || !row_len) {
    snprintf(g_err, sizeof(g_err), "bert_embed_ragged: unsupported shape (H=%d, max_T=%d, stride=%d)", H, max_T, ids_stride);
    return 1;
  }
  dim3 grid(cdiv((long)n * max_T, 4)), block(256);
  if (prec == PREC_BF16)
    hipLaunchKernelGGL(bert_embed_ragged_kernel<bf16_t>, grid, block, 0, st, ids, ids_stride, run, row_off, row_len, n, max_T, H, word, pos,
                       type0, gamma, beta, eps, (bf16_t*)y_act, y_f32);
  else if (prec == PREC_F16)
    hipLaunchKernelGGL(bert_embed_ragged_kernel<f16_t>, grid, block, 0, st, ids, ids_stride, run, row_off, row_len, n, max_T, H, word, pos,
                       type0, gamma, beta, eps, (f16_t*)y_act, y_f32);
  else if (prec == PREC_F16X3)
    hipLaunchKernelGGL(bert_embed_ragged_kernel<split_t>, grid, block, 0, st, ids, ids_stride, run, row_off, row_len, n, max_T, H, word, pos,
                       type0, gamma, beta, eps, (split_t*)y_act, y_f32);
  else
    hipLaunchKernelGGL(bert_embed_ragged_kernel<float>, grid, block, 0, st, ids, ids_stride, run, row_off, row_len, n, max_T, H, word, pos,
                       type0, gamma, beta, eps, (float*)y_act, y_f32);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

// packed row row_off[b] + gen[b]: the one row of sequence b that bert_prune keeps and the MLM head reads
__global__ void ragged_row_index_kernel(int* idx, int n, const int* row_off, const int* gen) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n) idx[b] = row_off[b] + gen[b];
}

int launch_ragged_row_index(int* idx, int n, const int* row_off, const int* gen, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(ragged_row_index_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, idx, n, row_off, gen);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace czc
