// Caption retrieval: a resident text index (czc_index_set) and its fused scan + top-k (czc_index_search).
//
// Storage.  Index rows and query rows are L2-normalised fp32 values in the split-fp16 row format of common.h (split_t: per 8
// elements 16 bytes of hi parts, then 16 bytes of lo parts), so an MFMA fragment of 8 consecutive k is one 16-byte load per plane.
//
// Scan (index_scan_kernel).  Work-groups of four waves are persistent and stride over 32-row blocks of the index; every wave owns
// whole blocks (all of D), so nothing is split along D.  A block is the A operand of v_mfma_f32_32x32x16_f16, the query tile (up
// to 32 queries, zero columns behind Q) the B operand, held in LDS in fragment order.  Per 16 k: lo.hi, hi.lo, hi.hi into ONE fp32
// accumulator, k ascending -- the score of a (query, row) pair is the same bits wherever the row or the query sits.
// Selection: the work-group keeps a sorted best-k list per query in LDS as 64-bit keys (order-preserving image of the cosine in
// the high word, ~id in the low word: key order = cosine descending, id ascending); a score is one compare against the list's
// k-th key, and only blocks in which some score passes take the insertion path.  The best-k SET under a total order does not
// depend on the order of insertion, so neither the wave that found a row nor the group count changes the result.
// Merge (index_merge_kernel): one work-group per query, G sorted partial lists -> k rounds of a block-wide max over the heads.
#include <algorithm>

#include "kernels.h"

namespace czc {

namespace {

constexpr int RT_THREADS = 256, RT_WAVES = 4;
constexpr unsigned long long RT_EMPTY = 0x007fffffull << 32;  // (-inf, id -1)

__device__ __forceinline__ unsigned long long rt_key(float cos, int id) {
  const unsigned u = __float_as_uint(cos);
  const unsigned o = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
  return ((unsigned long long)o << 32) | (unsigned)~id;
}
__device__ __forceinline__ float rt_key_cos(unsigned long long key) {
  const unsigned o = (unsigned)(key >> 32);
  return __uint_as_float((o >> 31) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ int rt_key_id(unsigned long long key) { return (int)~(unsigned)key; }

// one wave per row: fp32 row -> normalised split_t row; bad[row * bad_stride] = 1 (or, bad_stride == 0, the one shared flag is
// raised) where the norm is 0 or not finite.  D % 32 == 0, D <= 1024.
__global__ void __launch_bounds__(RT_THREADS) normalize_split_kernel(const float* __restrict__ src, long n, int D, split_t* __restrict__ dst,
                                                                      int* __restrict__ bad, int bad_stride) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * RT_WAVES + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* s = src + row * D;
  float4 v[LN_MAXV];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < D) {
      v[i] = *(const float4*)(s + c);
      ss += ln_sq4(v[i].x, v[i].y, v[i].z, v[i].w);
    }
  }
  ss = wave_sum(ss);
  const bool ok = ss > 0.f && ss < INFINITY;  // false for NaN as well
  if (lane == 0) {
    if (bad_stride) bad[row * bad_stride] = ok ? 0 : 1;
    else if (!ok) *bad = 1;
  }
  const float inv = ok ? 1.0f / sqrtf(ss) : 0.f;
  split_t* d = dst + row * D;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) Act<split_t>::st4(d, c, ok ? v[i].x * inv : 0.f, ok ? v[i].y * inv : 0.f, ok ? v[i].z * inv : 0.f, ok ? v[i].w * inv : 0.f);
  }
}

struct Frag { uint4 hi, lo; };

// KC: k-steps (of 16) per register chunk; a chunk of the next block is in flight while one is multiplied
template <int KC>
__global__ void __launch_bounds__(RT_THREADS, 2) index_scan_kernel(const split_t* __restrict__ index, int n, int D,
                                                                    const split_t* __restrict__ queries, int Q, int k,
                                                                    unsigned long long* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rt_smem[];
  const int KS = D >> 4;                                                   // k-steps per row
  uint4* q_hi = (uint4*)rt_smem;                                           // [KS][64]
  uint4* q_lo = q_hi + (size_t)KS * 64;                                    // [KS][64]
  unsigned long long* list = (unsigned long long*)(q_lo + (size_t)KS * 64);  // [32][k], descending
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const int G = gridDim.x, g = blockIdx.x, q0 = blockIdx.y * 32;
  const int Qt = min(32, Q - q0);
  const size_t row_b = (size_t)D * 4;

  for (int i = tid; i < KS * 64; i += RT_THREADS) {
    const int s = i >> 6, l = i & 63, j = l & 31, h = l >> 5;
    uint4 hi = make_uint4(0, 0, 0, 0), lo = hi;
    if (j < Qt) {
      const unsigned char* p = (const unsigned char*)queries + (size_t)(q0 + j) * row_b + (size_t)(2 * s + h) * 32;
      hi = *(const uint4*)p;
      lo = *(const uint4*)(p + 16);
    }
    q_hi[i] = hi;
    q_lo[i] = lo;
  }
  for (int i = tid; i < 32 * k; i += RT_THREADS) list[i] = RT_EMPTY;
  __syncthreads();

  const int nblocks = (n + 31) >> 5;
  const int stride = G * RT_WAVES;
  const int iters = (nblocks + stride - 1) / stride;
  const int chunks = KS / KC;
  auto row_ptr = [&](int it) -> const unsigned char* {
    const int b = min(it * stride + g * RT_WAVES + wave, nblocks - 1);   // clamped: a wave without a block re-reads the last one
    const int row = min(b * 32 + col, n - 1);                            // and ignores it; rows >= n are never addressed
    return (const unsigned char*)index + (size_t)row * row_b + half * 32;
  };
  auto load = [&](Frag (&f)[KC], const unsigned char* p, int c) {
#pragma unroll
    for (int s = 0; s < KC; ++s) {
      const unsigned char* a = p + (size_t)(c * KC + s) * 64;
      f[s].hi = *(const uint4*)a;
      f[s].lo = *(const uint4*)(a + 16);
    }
  };

  Frag cur[KC], nxt[KC];
  const unsigned char* p = row_ptr(0);
  load(cur, p, 0);
  unsigned long long* mine = list + col * k;
  for (int it = 0; it < iters; ++it) {
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const unsigned char* pn = it + 1 < iters ? row_ptr(it + 1) : p;
    for (int c = 0; c < chunks; ++c) {
      const bool last = c + 1 == chunks;
      if (!last) load(nxt, p, c + 1);
      else load(nxt, pn, 0);  // behind the last block: one chunk of it again, unused
#pragma unroll
      for (int s = 0; s < KC; ++s) {
        const int qi = (c * KC + s) * 64 + lane;
        const uint4 bh = q_hi[qi], bl = q_lo[qi];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, cur[s].lo), __builtin_bit_cast(f16x8_t, bh), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, cur[s].hi), __builtin_bit_cast(f16x8_t, bl), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, cur[s].hi), __builtin_bit_cast(f16x8_t, bh), acc, 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < KC; ++s) cur[s] = nxt[s];
    }
    p = pn;

    // acc[r]: query `col` against row (r & 3) + 8 * (r >> 2) + 4 * half of this wave's block
    const int blk = it * stride + g * RT_WAVES + wave;
    const int row0 = blk * 32 + 4 * half;
    const bool live = blk < nblocks && col < Qt;
    const unsigned long long thr = mine[k - 1];
    unsigned long long key[16];
    bool pass = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + (r & 3) + 8 * (r >> 2);
      key[r] = live && row < n ? rt_key(acc[r], row) : 0ull;  // 0 < RT_EMPTY: excluded by the row index, whatever the score
      pass |= key[r] > thr;
    }
    if (__syncthreads_or(pass)) {
      // rare after the first blocks: one (wave, half) at a time, one lane per query inserts into that query's list
      for (int ph = 0; ph < 2 * RT_WAVES; ++ph) {
        if (ph == 2 * wave + half && pass) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const unsigned long long kk = key[r];
            if (kk > mine[k - 1]) {
              int i = k - 1;
              while (i > 0 && mine[i - 1] < kk) { mine[i] = mine[i - 1]; --i; }
              mine[i] = kk;
            }
          }
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < Qt * k; i += RT_THREADS) {
    const int q = i / k, j = i - q * k;
    part[((size_t)(q0 + q) * G + g) * k + j] = list[q * k + j];
  }
}

// one work-group per query: G descending lists of k keys -> the k largest keys, descending
constexpr int RT_MERGE_LISTS = 4;  // lists per thread: G <= 1024
__global__ void __launch_bounds__(RT_THREADS) index_merge_kernel(const unsigned long long* __restrict__ part, int G, int k,
                                                                  int* __restrict__ out_ids, float* __restrict__ out_cos) {
  __shared__ unsigned long long red[2][RT_WAVES];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long* base = part + (size_t)q * G * k;
  int head[RT_MERGE_LISTS];
  unsigned long long top[RT_MERGE_LISTS];
#pragma unroll
  for (int i = 0; i < RT_MERGE_LISTS; ++i) {
    const int l = tid + i * RT_THREADS;
    head[i] = 0;
    top[i] = l < G ? base[(size_t)l * k] : 0ull;
  }
  for (int j = 0; j < k; ++j) {
    unsigned long long m = 0ull;
#pragma unroll
    for (int i = 0; i < RT_MERGE_LISTS; ++i) m = top[i] > m ? top[i] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(m, o, 64);
      m = other > m ? other : m;
    }
    if (lane == 0) red[j & 1][wave] = m;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < RT_WAVES; ++w) m = red[j & 1][w] > m ? red[j & 1][w] : m;
    if (m < RT_EMPTY) m = RT_EMPTY;
    if (tid == 0) {
      out_ids[(size_t)q * k + j] = rt_key_id(m);
      out_cos[(size_t)q * k + j] = rt_key_cos(m);
    }
    if (m != RT_EMPTY) {  // ids are unique across the lists: exactly one head holds m
#pragma unroll
      for (int i = 0; i < RT_MERGE_LISTS; ++i) {
        if (top[i] == m) {
          const int l = tid + i * RT_THREADS;
          ++head[i];
          top[i] = head[i] < k ? base[(size_t)l * k + head[i]] : 0ull;
        }
      }
    }
  }
}

constexpr int RT_MAX_DYN_LDS = 159 * 1024;
size_t scan_lds_bytes(int D, int k) { return (size_t)D * 128 + (size_t)32 * k * 8; }

template <int KC>
int launch_scan_t(const split_t* index, int n, int D, const split_t* queries, int Q, int k, int G, unsigned long long* part,
                  hipStream_t st) {
  static PerDeviceInit per_dev;
  const LaunchInit li = per_dev.get([](LaunchInit&) -> int {
    // (the kernel has a few hundred bytes of static LDS of its own -- the work-group vote -- so not the full 160 KiB)
    CZC_HIP_CHECK(hipFuncSetAttribute((const void*)index_scan_kernel<KC>, hipFuncAttributeMaxDynamicSharedMemorySize, RT_MAX_DYN_LDS));
    return 0;
  });
  if (li.rc) return launch_init_failed("index scan");
  hipLaunchKernelGGL((index_scan_kernel<KC>), dim3(G, cdiv(Q, 32)), dim3(RT_THREADS), scan_lds_bytes(D, k), st, index, n, D,
                     queries, Q, k, part);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

int launch_normalize_split(const float* src, long n, int D, split_t* dst, int* bad, int bad_stride, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(normalize_split_kernel, dim3(cdiv(n, RT_WAVES)), dim3(RT_THREADS), 0, st, src, n, D, dst, bad, bad_stride);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

// work-groups of the scan: `groups` as given (option "index_groups", 1..1024), or, 0, one per four blocks up to what the
// device holds at once (two work-groups per CU while their LDS allows it)
int index_scan_groups(int n, int D, int k, int groups) {
  static PerDeviceInit per_dev;
  if (groups <= 0) {
    const LaunchInit li = per_dev.get([](LaunchInit&) -> int { return 0; });
    const int n_cu = li.rc == 0 && li.n_cu > 0 ? li.n_cu : 256;
    groups = std::min(cdiv((n + 31) / 32, RT_WAVES), n_cu * (scan_lds_bytes(D, k) > 80 * 1024 ? 1 : 2));
  }
  return std::max(1, std::min(groups, RT_MERGE_LISTS * RT_THREADS));
}

// part: Q x G x k keys, G = index_scan_groups(n, D, k, groups)
int launch_index_search(const split_t* index, int n, int D, const split_t* queries, int Q, int k, int G,
                        unsigned long long* part, int* out_ids, float* out_cos, hipStream_t st) {
  if (D % 32 || D > 1024 || scan_lds_bytes(D, k) > (size_t)RT_MAX_DYN_LDS || G < 1 || G > RT_MERGE_LISTS * RT_THREADS || k < 1 || k > 64) {
    snprintf(g_err, sizeof(g_err), "index scan: bad shape D = %d, groups = %d, k = %d", D, G, k);
    return 1;
  }
  const int rc = (D % 128 == 0) ? launch_scan_t<8>(index, n, D, queries, Q, k, G, part, st)
                                : launch_scan_t<2>(index, n, D, queries, Q, k, G, part, st);
  if (rc) return rc;
  hipLaunchKernelGGL(index_merge_kernel, dim3(Q), dim3(RT_THREADS), 0, st, part, G, k, out_ids, out_cos);
  CZC_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace czc
