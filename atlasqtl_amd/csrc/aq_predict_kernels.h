// aq_predict_kernels.h -- Yhat = Xt B, the fitted model applied to rows of genotypes: B = gam * mu
// (p x q) read where it lies in the trait-tiled layout [tile][p_pad][16], Xt the standardised rows.  Included by
// aq_predict.hip only; the launch plan is aq_predict_plan.h.  Every kernel is a plain grid: no workgroup waits for another one,
// nothing spins, no LDS is shared between waves of the product kernel and no floating-point atomic is used, so two calls give
// the same bits.  Every offset is 64-bit.
//
// MFMA operands (v_mfma_f64_16x16x4_f64): A and B hold one f64 per lane, lane = 16 k + index (k = position within the step
// of 4 predictors); the accumulator has col = lane & 15 (the B index: the trait) and row = (lane >> 4) + 4 reg (the A index:
// the sample): the layout aq_probe_dmode verifies on the device, which the entries require before they launch.
//
// Both operands lie in the same order, [tile of 16][p_pad][16]: the 16 values of predictor j are 128 contiguous bytes, so the
// operand of the step (j0 ... j0 + 3) is the 64 doubles from (tile p_pad + j0) 16 on, element `lane` for lane `lane` -- one
// 512-byte run per load instruction, and a 16 x 16 block of B is 2 KB contiguous in gam and in mu.
//
// aq_k_predict_pack<T>: the rows of X (n rows x p, column-major with leading dimension ld, fp64 or int8) -> the panels Xp
// [n_pad / 16][p_pad][16] of Xt = (x - center) inv_scale (center == nullptr: x as it is), with exact 0.0 in the rows >= n and
// the predictors >= p.  Grid (p_pad / 16, sample tiles of this launch), 256 threads: one thread per element of Xp, 16
// consecutive threads read 16 consecutive samples of a column; the host launches it over ranges of sample tiles from it0 on,
// so that no launch has more than 2^30 threads.
//
// aq_k_predict_partial<NS, TT, HAS_MU>, grid (sample_blocks, trait_groups, splits), 256 threads: wave w of workgroup (b, g, s)
// owns the sample tiles (4 b + w) NS ... + NS - 1 and the trait tiles g TT ... + TT - 1 and walks the predictors
// [s cps 16, (s + 1) cps 16) below p, 16 at a time: it loads the four steps of gam and mu of its trait tiles, forms
// B = gam mu in registers -- a predictor >= p, a trait >= q or a tile >= ceil(q / 16) gives 0.0 by selection, never by
// multiplication, so what the padding of the storage holds (zeros, NaN, anything) cannot reach the result -- and multiplies
// every block of B with its NS sample tiles: NS x TT accumulators.  The operands of the next chunk are requested before the
// current one is multiplied.  All loads stay inside the allocations whatever they are masked to: a chunk's 16 predictors lie
// below p_pad, and the tile index is clamped to the last one.  The partial tile goes to
// scratch[((s tiles_q + tile) n_pad + 16 it) 16 + 64 reg + lane]: 512 contiguous bytes per store instruction.  A split
// without predictors stores zeros.  A tile >= tiles_q is not stored.
//
// aq_k_predict_reduce, grid (ceil(n_pad / 64), tiles_q), 256 threads: adds the partials of an entry in the order s = 0, 1, ...
// and writes Yhat[k n + i] for i < n, k < q through an LDS transpose, so that reads and writes are both contiguous.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aq_predict_plan.h"

typedef double aq_pred_d4 __attribute__((ext_vector_type(4)));

template <typename T>
__global__ __launch_bounds__(256) void aq_k_predict_pack(const T *__restrict__ X, long long ld, int n, int p, long long p_pad,
                                                        const double *__restrict__ center, const double *__restrict__ inv_scale,
                                                        int it0, double *__restrict__ Xp) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;        // element of the tile's panel: 16 p_pad = 256 gridDim.x
  const long long it = (long long)it0 + blockIdx.y, j = e >> 4, i = 16 * it + (e & 15);
  double v = 0.0;
  if (i < (long long)n && j < (long long)p) {
    v = (double)X[(size_t)i + (size_t)ld * (size_t)j];
    if (center) v = (v - center[j]) * inv_scale[j];
  }
  Xp[(size_t)it * (size_t)p_pad * 16 + (size_t)e] = v;
}

template <int NS, int TT, bool HAS_MU>
__global__ __launch_bounds__(256) void aq_k_predict_partial(const double *__restrict__ Xp, const double *__restrict__ gam,
                                                           const double *__restrict__ mu, int p, int q, long long p_pad, int n_pad,
                                                           int tiles_q, int cps, double *__restrict__ scratch) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, l = lane & 15;
  const long long j_begin = (long long)blockIdx.z * cps * AQ_PREDICT_KC;
  const long long j_end = min((long long)p, j_begin + (long long)cps * AQ_PREDICT_KC);
  const int it0 = (4 * (int)blockIdx.x + w) * NS;               // the wave's first sample tile; all NS lie below n_pad / 16
  const double *xa[NS];
#pragma unroll
  for (int u = 0; u < NS; u++) xa[u] = Xp + (size_t)(it0 + u) * (size_t)p_pad * 16 + lane;
  const double *gb[TT], *mb[TT];
  bool live[TT];                                                // this lane's trait exists
  int tile[TT];
#pragma unroll
  for (int t = 0; t < TT; t++) {
    tile[t] = (int)blockIdx.y * TT + t;
    live[t] = tile[t] < tiles_q && 16 * tile[t] + l < q;
    const int tc = min(tile[t], tiles_q - 1);                   // a tile that does not exist is read as the last one and masked
    gb[t] = gam + (size_t)tc * (size_t)p_pad * 16 + lane;
    mb[t] = HAS_MU ? mu + (size_t)tc * (size_t)p_pad * 16 + lane : nullptr;
  }
  aq_pred_d4 acc[NS][TT];
#pragma unroll
  for (int u = 0; u < NS; u++)
#pragma unroll
    for (int t = 0; t < TT; t++) acc[u][t] = aq_pred_d4{0.0, 0.0, 0.0, 0.0};
  double va[NS][4], vg[TT][4], vm[TT][4];
  auto load = [&](long long j0) {                               // j0 < p is a multiple of 16: j0 + 15 < p_pad
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      const size_t off = (size_t)(j0 + 4 * kk) * 16;
#pragma unroll
      for (int u = 0; u < NS; u++) va[u][kk] = xa[u][off];
#pragma unroll
      for (int t = 0; t < TT; t++) {
        vg[t][kk] = gb[t][off];
        vm[t][kk] = HAS_MU ? mb[t][off] : 1.0;
      }
    }
  };
  if (j_begin < j_end) load(j_begin);
  for (long long j0 = j_begin; j0 < j_end; j0 += AQ_PREDICT_KC) {
    double a[NS][4], b[TT][4];
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      const bool in_p = j0 + 4 * kk + g < (long long)p;
#pragma unroll
      for (int u = 0; u < NS; u++) a[u][kk] = va[u][kk];
#pragma unroll
      for (int t = 0; t < TT; t++) b[t][kk] = (in_p && live[t]) ? vg[t][kk] * vm[t][kk] : 0.0;
    }
    if (j0 + AQ_PREDICT_KC < j_end) load(j0 + AQ_PREDICT_KC);
#pragma unroll
    for (int kk = 0; kk < 4; kk++)
#pragma unroll
      for (int t = 0; t < TT; t++)
#pragma unroll
        for (int u = 0; u < NS; u++) acc[u][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][kk], b[t][kk], acc[u][t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < TT; t++) {
    if (tile[t] >= tiles_q) continue;
    double *out = scratch + (((size_t)blockIdx.z * (size_t)tiles_q + (size_t)tile[t]) * (size_t)n_pad) * 16 + lane;
#pragma unroll
    for (int u = 0; u < NS; u++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) out[(size_t)(it0 + u) * 256 + 64 * reg] = acc[u][t][reg];
  }
}

__global__ __launch_bounds__(256) void aq_k_predict_reduce(const double *__restrict__ scratch, int splits, int tiles_q, int n_pad, int n,
                                                          int q, double *__restrict__ Y) {
  __shared__ double buf[16][65];
  const int tile = blockIdx.y, r0 = 64 * (int)blockIdx.x;
  const size_t per_split = (size_t)tiles_q * (size_t)n_pad * 16;
  for (int e = threadIdx.x; e < 16 * 64; e += 256) {
    const int rr = e >> 4, k = e & 15, r = r0 + rr;
    double v = 0.0;
    if (r < n_pad) {
      const double *src = scratch + ((size_t)tile * (size_t)n_pad + (size_t)r) * 16 + k;
      for (int s = 0; s < splits; s++) v += src[(size_t)s * per_split];
    }
    buf[k][rr] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 16 * 64; e += 256) {
    const int k = e >> 6, rr = e & 63, kk = 16 * tile + k, r = r0 + rr;
    if (kk < q && r < n) Y[(size_t)r + (size_t)n * (size_t)kk] = buf[k][rr];
  }
}
