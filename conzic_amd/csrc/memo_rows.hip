// Per-row step memo of czc_generate_rows (option "memo_rows", engine.hip): the rule of memo.hip keyed per ROW.  Row r visits
// its own column at every step, so its entry is addressed by (r, first position of the step group): at most L slots per row.
// A slot carries a valid word (cleared at the start of the call) and a signature word (the group's n_mask and length and the
// column of its second step), so a first visit and a visit with another group shape are misses.
//
// Slot (p, r), p = first position of the group, e = p * R + r:  valid[e], sig[e], key[e][T] (the masked row R(r) of the last
// visit), and per sub-step j < MEMO_ROWS_SUB with f = (p * MEMO_ROWS_SUB + j) * R + r:  rows[f][T] (the row the sub-step
// left), cos[f] (winner cosine), imax[f] (longest CLIP branch of the plan).
//
// czc_generate_rows_from: a row that sits a step group out carries CZC_POS_IDLE in place of its column in the schedule slice
// (col0[r] < 0).  It is neither a hit nor a miss: hit[r] = MR_IDLE keeps it off the active list and away from its slots.
#include "../../include/conzic_hip.h"
#include "kernels.h"

namespace czc {

constexpr int MR_MISS = 0, MR_HIT = 1, MR_IDLE = 2;  // hit[r] as the flag kernel leaves it

__device__ __forceinline__ int mr_masked(const int* row, int t, int col, int n_mask, int mask_id) {
  return (t >= col && t < col + n_mask) ? mask_id : row[t];
}

// slot position of row r, or -1 where the column lies outside the caption (the host checks positions; nothing is addressed then)
__device__ __forceinline__ int mr_pos(const MemoRowsTab& m, const int* col0, int r) {
  const int p = col0[r] - m.seed_len;
  return (p >= 0 && p < m.L) ? p : -1;
}

__device__ __forceinline__ int mr_sig(int n_mask0, int n_sub, const int* col1, int r) {
  return (n_mask0 & 0xff) | (n_sub << 8) | ((n_sub > 1 && col1 ? col1[r] + 1 : 0) << 16);
}

// Check, first half.  One thread per row, 256 rows per work-group, R / 256 work-groups: the comparison reads 2 x T ints per row
// (8 MB at R = 16384, T = 64), which one work-group walking the batch would pull through a single CU.  Thread r compares
// R(r), built on the fly from the step's schedule slice, with the key row of r's own slot; hit[r] = 1 where valid, signature
// and every column agree, MR_IDLE where the row sits the group out.  cnt[work-group] = its rows that run (MR_MISS); tot[1 + j] (zeroed by the launcher) = longest branch
// a hit row had at sub-step j on its last visit.
__global__ __launch_bounds__(256) void memo_rows_flag_kernel(const int* inp, MemoRowsTab m, const int* col0, const int* col1,
                                                             int n_mask0, int n_sub, int mask_id, const RowDraw* draw_rows, int* hit,
                                                             int* cnt, int* tot) {
  __shared__ int wcount[4];
  __shared__ int hmax[MEMO_ROWS_SUB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = blockIdx.x * 256 + tid;
  if (tid < MEMO_ROWS_SUB) hmax[tid] = 0;
  __syncthreads();
  int act = 0;
  if (r < m.R) {
    const bool idle = col0[r] < 0;
    const int p = idle ? -1 : mr_pos(m, col0, r);
    bool same = false;
    if (p >= 0) {
      const size_t e = (size_t)p * m.R + r;
      same = m.valid[e] == 1 && m.sig[e] == mr_sig(n_mask0, n_sub, col1, r);
      if (draw_rows && draw_rows[r].tau > 0.f) same = false;  // a row that draws its winner always runs (czc_generate_rows_draw)
      if (same) {
        const int* row = inp + (size_t)r * m.T;
        const int* k = m.key + e * m.T;
        const int c = col0[r];
        for (int t = 0; t < m.T && same; ++t) same = mr_masked(row, t, c, n_mask0, mask_id) == k[t];
      }
      if (same)
        for (int j = 0; j < n_sub && j < MEMO_ROWS_SUB; ++j) {
          const int v = m.imax[((size_t)p * MEMO_ROWS_SUB + j) * m.R + r];
          if (v > 0) atomicMax(&hmax[j], v);
        }
    }
    hit[r] = idle ? MR_IDLE : same ? MR_HIT : MR_MISS;
    act = (idle || same) ? 0 : 1;
  }
  const unsigned long long b = __ballot(act);
  if (lane == 0) wcount[w] = __popcll(b);
  __syncthreads();
  if (tid == 0) cnt[blockIdx.x] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
  if (tid < MEMO_ROWS_SUB && hmax[tid] > 0) atomicMax(&tot[1 + tid], hmax[tid]);
}

// Check, second half: the rows that run (neither hit nor idle), in ascending order.  Work-group g adds up the counts of the work-groups in
// front of it (at most CZC_MAX_ROWS / 256 = 64 words), ranks its own rows by wave ballot, and the last one writes the total.
__global__ __launch_bounds__(256) void memo_rows_list_kernel(const int* hit, int R, const int* cnt, int* list, int* tot) {
  __shared__ int wcount[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = blockIdx.x * 256 + tid;
  int base = 0;
  for (int i = 0; i < (int)blockIdx.x; ++i) base += cnt[i];
  const int act = (r < R && hit[r] == MR_MISS) ? 1 : 0;
  const unsigned long long b = __ballot(act);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wcount[w] = __popcll(b);
  __syncthreads();
  int off = base;
  for (int i = 0; i < w; ++i) off += wcount[i];
  if (act) list[off + before] = r;
  if (blockIdx.x == gridDim.x - 1 && tid == 0) tot[0] = base + wcount[0] + wcount[1] + wcount[2] + wcount[3];
}

int launch_memo_rows_check(const int* inp, const MemoRowsTab& m, const int* col0, const int* col1, int n_mask0, int n_sub,
                           int mask_id, int* hit, int* cnt, int* list, int* tot, hipStream_t st, const RowDraw* draw_rows) {
  if (m.R <= 0 || m.R > CZC_MAX_ROWS) { snprintf(g_err, sizeof(g_err), "memo_rows check: bad row count %d", m.R); return 1; }
  const int nb = (m.R + 255) / 256;
  CZC_HIP_CHECK(hipMemsetAsync(tot, 0, 16, st));
  hipLaunchKernelGGL(memo_rows_flag_kernel, dim3(nb), dim3(256), 0, st, inp, m, col0, col1, n_mask0, n_sub, mask_id, draw_rows, hit, cnt, tot);
  CZC_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(memo_rows_list_kernel, dim3(nb), dim3(256), 0, st, hit, m.R, cnt, list, tot);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

// One work-group per listed row i (row r = list[i]; list == null: r = i).  record: R(r) becomes the key row of r's slot, which
// turns valid with this group's signature.  inp_c != null: row r -> compact row i, its normalised image embed -> compact
// embed i, and its column / '.' rule of THIS step (col / dot: the step's schedule slice) -> compact entries i.
__global__ __launch_bounds__(256) void memo_rows_gather_kernel(const int* inp, const int* list, MemoRowsTab m, const int* col0,
                                                               const int* col1, int n_mask0, int n_sub, int mask_id, int record,
                                                               const int* col, const int* dot, int* inp_c, const float* img_n,
                                                               int D, float* img_c, int* col_c, int* dot_c) {
  const int i = blockIdx.x;
  const int r = list ? list[i] : i;
  if (r < 0 || r >= m.R) return;
  const int* row = inp + (size_t)r * m.T;
  const int p = record ? mr_pos(m, col0, r) : -1;
  const int c0 = col0[r];
  int* k = p >= 0 ? m.key + ((size_t)p * m.R + r) * m.T : nullptr;
  for (int t = threadIdx.x; t < m.T; t += blockDim.x) {
    if (k) k[t] = mr_masked(row, t, c0, n_mask0, mask_id);
    if (inp_c) inp_c[(size_t)i * m.T + t] = row[t];
  }
  if (threadIdx.x == 0) {
    if (p >= 0) { m.valid[(size_t)p * m.R + r] = 1; m.sig[(size_t)p * m.R + r] = mr_sig(n_mask0, n_sub, col1, r); }
    if (inp_c) { col_c[i] = col[r]; dot_c[i] = dot[r]; }
  }
  if (inp_c)
    for (int d = threadIdx.x; d < D; d += blockDim.x) img_c[(size_t)i * D + d] = img_n[(size_t)r * D + d];
}

int launch_memo_rows_gather(const int* inp, const int* list, int n, const MemoRowsTab& m, const int* col0, const int* col1,
                            int n_mask0, int n_sub, int mask_id, int record, const int* col, const int* dot, int* inp_c,
                            const float* img_n, int D, float* img_c, int* col_c, int* dot_c, hipStream_t st) {
  if (n <= 0) return 0;
  if (n > m.R) { snprintf(g_err, sizeof(g_err), "memo_rows gather: %d rows of %d", n, m.R); return 1; }
  hipLaunchKernelGGL(memo_rows_gather_kernel, dim3(n), dim3(256), 0, st, inp, list, m, col0, col1, n_mask0, n_sub, mask_id, record,
                     col, dot, inp_c, img_n, D, img_c, col_c, dot_c);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

// After sub-step j on n rows: work-group i takes row i of `rows` (the compact rows, or the full batch when list == null) and
// its winner cosine; row r = list[i] (or i).  With a list the row goes back into inp[r]; the cosine goes to bcos_full[r];
// record: row, cosine and longest branch become sub-step j of r's slot.
__global__ __launch_bounds__(256) void memo_rows_scatter_kernel(const int* rows, const float* bcos, const int* img_max,
                                                                const int* list, MemoRowsTab m, const int* col0, int j, int record,
                                                                int* inp, float* bcos_full) {
  const int i = blockIdx.x;
  const int r = list ? list[i] : i;
  if (r < 0 || r >= m.R) return;
  const int p = record ? mr_pos(m, col0, r) : -1;
  const size_t f = p >= 0 ? ((size_t)p * MEMO_ROWS_SUB + j) * m.R + r : 0;
  const int* src = rows + (size_t)i * m.T;
  for (int t = threadIdx.x; t < m.T; t += blockDim.x) {
    const int v = src[t];
    if (list) inp[(size_t)r * m.T + t] = v;
    if (p >= 0) m.rows[f * m.T + t] = v;
  }
  if (threadIdx.x == 0) {
    const float c = bcos[i];
    bcos_full[r] = c;
    if (p >= 0) { m.cos[f] = c; m.imax[f] = img_max[i]; }
  }
}

int launch_memo_rows_scatter(const int* rows, const float* bcos, const int* img_max, const int* list, int n, const MemoRowsTab& m,
                             const int* col0, int j, int record, int* inp, float* bcos_full, hipStream_t st) {
  if (n <= 0) return 0;
  if (n > m.R || (record && (j < 0 || j >= MEMO_ROWS_SUB))) { snprintf(g_err, sizeof(g_err), "memo_rows scatter: bad n / sub-step"); return 1; }
  hipLaunchKernelGGL(memo_rows_scatter_kernel, dim3(n), dim3(256), 0, st, rows, bcos, img_max, list, m, col0, j, record, inp,
                     bcos_full);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

// The hit rows of sub-step j: work-group r writes the row and cosine of its own slot back (for an n_mask = 1 group the row is
// the one it already has).
__global__ __launch_bounds__(64) void memo_rows_fill_kernel(const int* hit, MemoRowsTab m, const int* col0, int j, int* inp,
                                                            float* bcos_full) {
  const int r = blockIdx.x;
  if (hit[r] != MR_HIT) return;  // a miss ran; an idle row keeps its ids and its last cosine
  const int p = mr_pos(m, col0, r);
  if (p < 0) return;
  const size_t f = ((size_t)p * MEMO_ROWS_SUB + j) * m.R + r;
  for (int t = threadIdx.x; t < m.T; t += blockDim.x) inp[(size_t)r * m.T + t] = m.rows[f * m.T + t];
  if (threadIdx.x == 0) bcos_full[r] = m.cos[f];
}

int launch_memo_rows_fill(const int* hit, const MemoRowsTab& m, const int* col0, int j, int* inp, float* bcos_full, hipStream_t st) {
  if (j < 0 || j >= MEMO_ROWS_SUB) { snprintf(g_err, sizeof(g_err), "memo_rows fill: bad sub-step"); return 1; }
  if (m.R <= 0) return 0;
  hipLaunchKernelGGL(memo_rows_fill_kernel, dim3(m.R), dim3(64), 0, st, hit, m, col0, j, inp, bcos_full);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace czc
