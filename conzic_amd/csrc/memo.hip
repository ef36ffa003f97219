// Exact step memo of czc_generate (option "memo", engine.hip): an image whose masked row at a (position, n_mask) key is the
// one it had on its last visit of that key gets the same winner and cosine again (the polishing rule is a deterministic
// argmax, gen_utils.py:66-79, and a caption does not depend on the batch it is polished in), so the step runs only for the
// images whose row changed, on a compact batch, and the others take the entry's row and cosine back.
//
// Entry layout (per key slot, laid out by engine.hip): key rows int32 [B][T] (the masked row R(b) of the last visit),
// and per sub-step j of the key's group (j = 0: the n_mask >= 1 step, j = 1: the n_mask = 0 step that re-uses its forward):
// out rows int32 [B][T] (the row the sub-step left), cosines fp32 [B] and the plan's longest branch int32 [B].
#include "kernels.h"

namespace czc {

// the row BERT sees: launch_mask_positions' columns gen_idx .. gen_idx + n_mask - 1 (inside the row) set to [MASK]
__device__ __forceinline__ int memo_masked(const int* row, int t, int gen_idx, int n_mask, int mask_id) {
  return (t >= gen_idx && t < gen_idx + n_mask) ? mask_id : row[t];
}

// One work-group of 256 threads (four waves) walks the batch 256 images at a time.  Thread b compares R(b), built on the
// fly, with the stored key row; the images that differ are listed in ascending order (wave ballot + a prefix over the four
// wave counts).  tot[0] = active count; tot[1 + j] = longest branch any HIT image had at sub-step j on its last visit.
__global__ __launch_bounds__(256) void memo_check_kernel(const int* inp, int B, int T, int gen_idx, int n_mask, int mask_id,
                                                         const int* key, const int* img_max, int n_sub, int* hit, int* list,
                                                         int* tot) {
  __shared__ int wcount[4];
  __shared__ int hmax[2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < 2) hmax[tid] = 0;
  __syncthreads();
  int base = 0;
  int my_max[2] = {0, 0};
  for (int b0 = 0; b0 < B; b0 += 256) {
    const int b = b0 + tid;
    int act = 0;
    if (b < B) {
      const int* r = inp + (size_t)b * T;
      const int* k = key + (size_t)b * T;
      bool same = true;
      for (int t = 0; t < T; ++t) same = same && memo_masked(r, t, gen_idx, n_mask, mask_id) == k[t];
      act = same ? 0 : 1;
      hit[b] = same ? 1 : 0;
      if (same)
        for (int j = 0; j < n_sub && j < 2; ++j) my_max[j] = max(my_max[j], img_max[(size_t)j * B + b]);
    }
    const unsigned long long m = __ballot(act);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[w] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int i = 0; i < w; ++i) off += wcount[i];
    if (act) list[off + before] = b;
    base += wcount[0] + wcount[1] + wcount[2] + wcount[3];
    __syncthreads();  // wcount is rewritten by the next chunk
  }
  if (my_max[0]) atomicMax(&hmax[0], my_max[0]);
  if (my_max[1]) atomicMax(&hmax[1], my_max[1]);
  __syncthreads();
  if (tid == 0) { tot[0] = base; tot[1] = hmax[0]; tot[2] = hmax[1]; tot[3] = 0; }
}

int launch_memo_check(const int* inp, int B, int T, int gen_idx, int n_mask, int mask_id, const int* key, const int* img_max,
                      int n_sub, int* hit, int* list, int* tot, hipStream_t st) {
  hipLaunchKernelGGL(memo_check_kernel, dim3(1), dim3(256), 0, st, inp, B, T, gen_idx, n_mask, mask_id, key, img_max, n_sub, hit,
                     list, tot);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

// One work-group per listed image i (image b = list[i]; list == null: b = i).  key != null: records R(b) as the entry's key
// row; inp_c != null: row b -> compact row i; img_c != null: normalised image embed b -> compact embed i.
__global__ __launch_bounds__(256) void memo_gather_kernel(const int* inp, const int* list, int T, int gen_idx, int n_mask,
                                                          int mask_id, int* key, int* inp_c, const float* img_n, int D,
                                                          float* img_c) {
  const int i = blockIdx.x;
  const int b = list ? list[i] : i;
  const int* r = inp + (size_t)b * T;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    if (key) key[(size_t)b * T + t] = memo_masked(r, t, gen_idx, n_mask, mask_id);
    if (inp_c) inp_c[(size_t)i * T + t] = r[t];
  }
  if (img_c)
    for (int d = threadIdx.x; d < D; d += blockDim.x) img_c[(size_t)i * D + d] = img_n[(size_t)b * D + d];
}

int launch_memo_gather(const int* inp, const int* list, int n, int T, int gen_idx, int n_mask, int mask_id, int* key, int* inp_c,
                       const float* img_n, int D, float* img_c, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(memo_gather_kernel, dim3(n), dim3(256), 0, st, inp, list, T, gen_idx, n_mask, mask_id, key, inp_c, img_n, D,
                     img_c);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

// After the step on n rows: work-group i takes row i of `rows` (the compact rows, or the full batch when list == null) and
// its winner cosine; image b = list[i] (or i).  With a list the row goes back into inp[b]; the cosine goes to the full-batch
// buffer bcos_full[b]; out_rows / out_cos / out_max (each may be null) record the entry of this sub-step.
__global__ __launch_bounds__(256) void memo_scatter_kernel(const int* rows, const float* bcos, const int* img_max, const int* list,
                                                           int T, int* inp, float* bcos_full, int* out_rows, float* out_cos,
                                                           int* out_max) {
  const int i = blockIdx.x;
  const int b = list ? list[i] : i;
  const int* r = rows + (size_t)i * T;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const int v = r[t];
    if (list) inp[(size_t)b * T + t] = v;
    if (out_rows) out_rows[(size_t)b * T + t] = v;
  }
  if (threadIdx.x == 0) {
    const float c = bcos[i];
    bcos_full[b] = c;
    if (out_cos) out_cos[b] = c;
    if (out_max) out_max[b] = img_max[i];
  }
}

int launch_memo_scatter(const int* rows, const float* bcos, const int* img_max, const int* list, int n, int T, int* inp,
                        float* bcos_full, int* out_rows, float* out_cos, int* out_max, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(memo_scatter_kernel, dim3(n), dim3(256), 0, st, rows, bcos, img_max, list, T, inp, bcos_full, out_rows,
                     out_cos, out_max);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

// The hit images of a step: work-group b writes the entry's row and cosine of this sub-step back (for an n_mask = 1 key the
// row is the one the image already has).
__global__ __launch_bounds__(64) void memo_fill_kernel(const int* hit, int T, const int* out_rows, const float* out_cos, int* inp,
                                                       float* bcos_full) {
  const int b = blockIdx.x;
  if (!hit[b]) return;
  for (int t = threadIdx.x; t < T; t += blockDim.x) inp[(size_t)b * T + t] = out_rows[(size_t)b * T + t];
  if (threadIdx.x == 0) bcos_full[b] = out_cos[b];
}

int launch_memo_fill(const int* hit, int B, int T, const int* out_rows, const float* out_cos, int* inp, float* bcos_full,
                     hipStream_t st) {
  if (B <= 0) return 0;
  hipLaunchKernelGGL(memo_fill_kernel, dim3(B), dim3(64), 0, st, hit, T, out_rows, out_cos, inp, bcos_full);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace czc
