// aq_ytrans_kernels.h -- the rank-based inverse normal transform of the traits (include/atlasqtl_hip.h, aq_rank_int and
// aq_prepare_data_opt; planned by aq_ytrans_plan.h), for gfx950.  Included by aq_prep_ytrans.hip, which sequences the kernels.
//
// One workgroup per trait.  The column's values become order-preserving 64-bit keys (aq_key_of_bits, -0.0 first made +0.0;
// NaN and the padding up to a power of two take ~0, above every value), the keys are sorted by a bitonic network, and every
// sample then finds lo = #keys below its own and hi = #keys <= its own by two binary searches in the sorted keys: its
// doubled average rank 2 r = lo + hi + 1 is an exact integer.  No index array is carried, ties need no extra pass and the
// result does not depend on the stability of the sort.  With m observed values and t = min(2 r, 2 m + 2 - 2 r) the output is
// -+ aq_ndtri((t - 2 c) / (2 m + 2 - 4 c)): ranks r and m + 1 - r give exact negatives, the middle rank exactly 0.
//   aq_k_yt_lds      the keys of the column in LDS (n_pad <= 16 384).
//   aq_k_yt_global   the keys of the column in device memory: chunks of min(n_pad, 16 384) keys are sorted in LDS, every
//                    stride of the network that fits a chunk runs there, the wider ones as passes over device memory.
// Both see the same sorted keys, so their outputs are bit-identical.  Plain HIP: vector loads and stores only, and every
// wait is a workgroup barrier -- a workgroup reads no key that another one wrote.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aq_internal.h"
#include "aq_special.h"        // aq_ndtri
#include "aq_ytrans_plan.h"

#define AQ_YT_BLOCK 1024
#define AQ_YT_KEY_NA 0xffffffffffffffffull   // a missing value and the padding: no value has this key (it is the key of a NaN)

__device__ __forceinline__ uint64_t aq_yt_key(double v) {
  if (v != v) return AQ_YT_KEY_NA;
  if (v == 0.0) v = 0.0;                       // -0.0 ties with +0.0
  return aq_key_of_bits((uint64_t)__double_as_longlong(v));
}

// the compare-exchange steps j = min(k / 2, cnt / 2) ... 1 of stage k of the network on the cnt keys s[] in LDS, which are
// the keys g0 ... g0 + cnt - 1 of the column (cnt a power of two that divides g0).  Ends on a barrier.
__device__ __forceinline__ void aq_yt_lds_steps(uint64_t *s, int cnt, int g0, int k) {
  const int half = cnt >> 1;
  for (int j = (k >> 1) < half ? (k >> 1) : half; j > 0; j >>= 1) {
    for (int t = threadIdx.x; t < half; t += blockDim.x) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // bit j clear
      const int l = i | j;
      const bool up = ((g0 + i) & k) == 0;
      const uint64_t a = s[i], b = s[l];
      if ((a > b) == up) { s[i] = b; s[l] = a; }
    }
    __syncthreads();
  }
}

// first index in the sorted keys s[0 .. cnt) (cnt a power of two) whose key is >= key (upper = false) or > key (upper = true)
template <bool UPPER>
__device__ __forceinline__ int aq_yt_bound(const uint64_t *s, int cnt, uint64_t key) {
  int pos = 0;                                 // keys before pos are below the bound
  for (int step = cnt >> 1; step > 0; step >>= 1) {
    const uint64_t v = s[pos + step - 1];
    if (UPPER ? v <= key : v < key) pos += step;
  }
  const uint64_t v = s[pos];                   // pos <= cnt - 1
  if (UPPER ? v <= key : v < key) pos += 1;
  return pos;
}

// the sorted keys of the column -> its transformed values and counts.  y and out may be the same array: a thread writes only
// the entries it has read itself.  cnt[0] / cnt[1]: LDS counters, zero on entry.
__device__ __forceinline__ void aq_yt_finish(const uint64_t *sorted, int n_pad, const double *y, int n, double c, double *out, int *cnt,
                                             int *nobs, int *ntied, int *degenerate) {
  const int m = aq_yt_bound<false>(sorted, n_pad, AQ_YT_KEY_NA);   // the observed values are the first m keys
  const double den = (double)(2 * m + 2) - 4.0 * c;
  int tied = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double v = y[i];
    double r = v;                              // NaN stays NaN
    if (v == v) {
      const uint64_t key = aq_yt_key(v);
      const int lo = aq_yt_bound<false>(sorted, n_pad, key), hi = aq_yt_bound<true>(sorted, n_pad, key);
      const int r2 = lo + hi + 1;              // twice the average rank
      const int mirror = 2 * m + 2 - r2;
      const int t = r2 < mirror ? r2 : mirror;
      const double x = aq_ndtri(((double)t - 2.0 * c) / den);
      r = r2 > mirror ? -x : x;
      tied += (hi - lo > 1);
    }
    out[i] = r;
  }
  if (tied) atomicAdd(&cnt[0], tied);
  __syncthreads();
  if (threadIdx.x == 0) {
    *nobs = m;
    *ntied = cnt[0];
    *degenerate = (m < 2 || sorted[0] == sorted[m - 1]) ? 1 : 0;
  }
}

// grid: one workgroup per trait; dynamic LDS: n_pad keys
__global__ __launch_bounds__(AQ_YT_BLOCK) void aq_k_yt_lds(const double *Y, int n, int n_pad, double c, double *out,
                                                          int *__restrict__ nobs, int *__restrict__ ntied, int *__restrict__ degenerate) {
  extern __shared__ uint64_t aq_yt_keys[];
  __shared__ int cnt[2];
  const size_t base = (size_t)blockIdx.x * n;
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  for (int i = threadIdx.x; i < n_pad; i += blockDim.x) aq_yt_keys[i] = i < n ? aq_yt_key(Y[base + i]) : AQ_YT_KEY_NA;
  __syncthreads();
  for (int k = 2; k <= n_pad; k <<= 1) aq_yt_lds_steps(aq_yt_keys, n_pad, 0, k);
  aq_yt_finish(aq_yt_keys, n_pad, Y + base, n, c, out + base, cnt, nobs + blockIdx.x, ntied + blockIdx.x, degenerate + blockIdx.x);
}

// grid: one workgroup per trait of the batch; dynamic LDS: chunk = min(n_pad, AQ_YT_LDS_KEYS) keys; keys: n_pad per workgroup
__global__ __launch_bounds__(AQ_YT_BLOCK) void aq_k_yt_global(const double *Y, int n, int n_pad, int chunk, double c, double *out,
                                                             uint64_t *keys, int *__restrict__ nobs, int *__restrict__ ntied,
                                                             int *__restrict__ degenerate) {
  extern __shared__ uint64_t aq_yt_keys[];
  __shared__ int cnt[2];
  const size_t base = (size_t)blockIdx.x * n;
  uint64_t *const g = keys + (size_t)blockIdx.x * n_pad;
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  // every chunk sorted on its own, in the direction the network gives it
  for (int g0 = 0; g0 < n_pad; g0 += chunk) {
    for (int i = threadIdx.x; i < chunk; i += blockDim.x) aq_yt_keys[i] = g0 + i < n ? aq_yt_key(Y[base + g0 + i]) : AQ_YT_KEY_NA;
    __syncthreads();
    for (int k = 2; k <= chunk; k <<= 1) aq_yt_lds_steps(aq_yt_keys, chunk, g0, k);
    for (int i = threadIdx.x; i < chunk; i += blockDim.x) g[g0 + i] = aq_yt_keys[i];
    __syncthreads();
  }
  // the stages that span several chunks: strides >= chunk on device memory, the rest of the stage chunk by chunk in LDS
  for (int k = chunk << 1; k <= n_pad; k <<= 1) {
    for (int j = k >> 1; j >= chunk; j >>= 1) {
      for (int t = threadIdx.x; t < (n_pad >> 1); t += blockDim.x) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const bool up = (i & k) == 0;
        const uint64_t a = g[i], b = g[l];
        if ((a > b) == up) { g[i] = b; g[l] = a; }
      }
      __syncthreads();
    }
    for (int g0 = 0; g0 < n_pad; g0 += chunk) {
      for (int i = threadIdx.x; i < chunk; i += blockDim.x) aq_yt_keys[i] = g[g0 + i];
      __syncthreads();
      aq_yt_lds_steps(aq_yt_keys, chunk, g0, k);
      for (int i = threadIdx.x; i < chunk; i += blockDim.x) g[g0 + i] = aq_yt_keys[i];
      __syncthreads();
    }
  }
  aq_yt_finish(g, n_pad, Y + base, n, c, out + base, cnt, nobs + blockIdx.x, ntied + blockIdx.x, degenerate + blockIdx.x);
}
