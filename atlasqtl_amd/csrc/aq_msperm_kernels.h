// aq_msperm_kernels.h -- permutation nulls of the marginal screen: the statistic of
// aq_mscreen_kernels.h evaluated on (Xs, Y') for permuted responses Y'[i, t] = Yc[perm[b][i], t], many permutations b per
// launch, keeping per permutation only the largest r^2 of every trait, the per-predictor counts of selected traits (on the
// device, reduced there to their maximum and their sum) and the number of undefined pairs.  Nothing of size p1 q exists and no
// pair table is written.  Included by aq_prep_marginal_perm.hip; the launch plan is aq_msperm_plan.h.  Every kernel is a plain
// grid: no workgroup waits for another one, nothing spins, and no floating-point atomic is used (the integer atomics are
// counters and a maximum over bit patterns), so two calls with the same arguments give the same bits in every output.
//
// aq_k_msperm_gather: Yp[b][t][i] = Yc[t][perm[b][i]] for the permutations of one launch.  A workgroup writes whole columns,
// 256 consecutive doubles at a time (coalesced); its scattered reads stay inside one column of Yc, 8 n bytes that sit in L2.
// NaN moves with the value: nothing is computed on it.  The host has checked that every index is in 0 ... n - 1.
// With Yp in the layout of Yc, [q][n] per permutation, the tile loop keeps the 16-byte loads, the LDS rows of 18 doubles and
// the bank argument of aq_k_ms_tile, and uses its aq_ms_load, aq_ms_store and aq_ms_store_masked.
//
// aq_k_msperm_tile<T, MASKED, A16, PB>, grid n_tiles groups, 256 threads.  Workgroup w owns the tile v = w mod n_tiles of
// predictors x traits exactly as aq_k_ms_tile owns it, and the permutations PB g ... PB g + PB - 1 of the launch, g = w /
// n_tiles.  Per chunk of 16 samples the panel of X is staged ONCE and multiplied against the PB panels of Y' (MASKED: also
// against the PB mask panels, three streams per permutation as in aq_k_ms_tile), into PB accumulator sets.  A 64 x 64 tile
// stages 2 x 64 columns for 64 x 64 outputs; with PB permutations it stages (1 + PB) x 64 columns for PB x 64 x 64 outputs:
// the traffic per output of a 64 x 64 PB tile, without a second set of X operands.  Every output element is accumulated over
// the samples in the order 0, 4, 8, ... of aq_k_ms_tile, one MFMA per step of 4, so the identity permutation reproduces its
// r to the bit.
// Registers (__launch_bounds__(256, 2): 256 a lane).  Accumulators: complete 2 (T / 32)^2 4 PB = 32 PB at T = 64 and 128 PB at
// T = 128; masked 96 PB.  With the staged loads (8 + 8 PB at T = 64) and the operands this admits complete T = 64 with
// PB <= 4, complete T = 128 with PB = 1 and masked (T = 64) with PB <= 2: aq_msperm_instance.  A permutation at or beyond the
// launch's count (the ragged last group) is neither loaded, multiplied nor written.
// Epilogue, in registers, per permutation: r^2 by the formula of aq_k_ms_tile; then
//   - the largest defined r^2 of a trait over the lane's predictors, across the sixteen lanes by xor shuffles, across the two
//     waves of a tile row through LDS, then ONE integer atomicMax per (permutation, trait) and workgroup on key = bits(r^2) + 1:
//     r^2 >= 0, so the order of the bit patterns is the order of the values, the maximum is exact and independent of the
//     order of arrival, and key 0 says that no pair of the trait is defined;
//   - the per-(permutation, predictor) count of selected traits by the route of aq_k_ms_tile: summed over the lane's traits,
//     over the four lane groups, then one integer atomic per predictor and wave where it is not zero;
//   - undefined pairs: counted per wave, one integer atomic per permutation.
//
// aq_k_msperm_reduce, grid = the launch's permutations, 256 threads: count[b][.] -> hs_max[b] (the largest) and n_sel[b] (the
// sum), integers added in a fixed order; key -> max_r2[b][t], -1.0 where the key is 0.
#pragma once
#include "aq_msperm_plan.h"
#include "aq_mscreen_kernels.h"   // aq_ms_d4, AqMsShape, aq_ms_load, aq_ms_store, aq_ms_store_masked

struct aq_msp_args {
  const double *Xs, *Yp;              // [p1][n], [nb][q][n]
  int n, p1, q, n_cov, tiles_p, n_tiles, nb;   // nb: the permutations of this launch
  const double *sx, *sxx;             // p1 each: the complete instance's Sx and Sxx
  const double *syy;                  // q
  const int *mt;                      // q
  const double *cut;                  // q: the cutoff on r^2
  unsigned long long *key;            // [nb][q]: bits(max r^2) + 1, 0: no defined pair
  unsigned int *count;                // [nb][p1]
  unsigned long long *n_undef;        // [nb]
};

__global__ __launch_bounds__(256) void aq_k_msperm_gather(const double *__restrict__ Yc, const int32_t *__restrict__ perm, int n, int q,
                                                         int nb, double *__restrict__ Yp) {
  const long long cols = (long long)nb * (long long)q;
  for (long long c = blockIdx.x; c < cols; c += gridDim.x) {
    const double *src = Yc + (size_t)(c % q) * (size_t)n;
    const int32_t *row = perm + (size_t)(c / q) * (size_t)n;
    double *dst = Yp + (size_t)c * (size_t)n;
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[row[i]];
  }
}

template <int T, bool MASKED, bool A16, int PB>
__global__ __launch_bounds__(256, 2) void aq_k_msperm_tile(const aq_msp_args a) {
  typedef AqMsShape<T> SH;
  static_assert(aq_msperm_instance(T, MASKED, PB), "an instance of the plan");
  constexpr int NI = SH::NI;
  constexpr int NS = MASKED ? NI : 1;                      // extent of the two extra accumulator sets (1: unused)
  constexpr int PAN = T * SH::STR;                         // doubles of a panel
  constexpr int YPAN = (MASKED ? 2 : 1) * PAN;             // per permutation: PY, then (MASKED) PM
  __shared__ __attribute__((aligned(16))) double PX[PAN];
  __shared__ __attribute__((aligned(16))) double PYM[PB * YPAN];
  __shared__ double ts_syy[T], ts_cut[T];                  // the tile's traits: Syy_t, the cutoff, and m_t (0 for a trait >= q)
  __shared__ int ts_m[T];
  __shared__ double cmax[2][PB][T];                        // per wave column: a trait's largest r^2 (-1.0: none)
  static_assert(sizeof(double) * (PAN + PB * YPAN) + T * 20 + sizeof(double) * 2 * PB * T == aq_msperm_lds_bytes(T, MASKED, PB),
                "plan and kernel");
  static_assert(aq_msperm_lds_bytes(T, MASKED, PB) <= 65536, "64 KB of static LDS");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, l = lane & 15;
  const int wr = w >> 1, wc = w & 1;
  const int v = (int)(blockIdx.x % (unsigned)a.n_tiles), grp = (int)(blockIdx.x / (unsigned)a.n_tiles);
  const int tp = v % a.tiles_p, tq = v / a.tiles_p;
  const int p0 = T * tp, q0 = T * tq;
  const int b0 = PB * grp;
  const int npb = a.nb - b0 < PB ? a.nb - b0 : PB;         // the group's permutations: >= 1 by the grid
  const int n = a.n;
  const size_t ystride = (size_t)a.q * (size_t)n;
  aq_ms_d4 axy[PB][NI][NI], ax[PB][NS][NS], axx[PB][NS][NS];
#pragma unroll
  for (int pb = 0; pb < PB; pb++) {
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
      for (int jj = 0; jj < NI; jj++) axy[pb][i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NS; i++)
#pragma unroll
      for (int jj = 0; jj < NS; jj++) {
        ax[pb][i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
        axx[pb][i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
      }
  }
  const int yoff = (wr * SH::WT + l) * SH::STR + g;        // the lane's first operand of Y' (and of the mask) within a panel
  const double *px = PX + (wc * SH::WT + l) * SH::STR + g;
  if ((int)threadIdx.x < T) {                      // read after the loop's barriers
    const int t = q0 + (int)threadIdx.x;
    const bool tv = t < a.q;
    ts_syy[threadIdx.x] = tv ? a.syy[t] : 0.0;
    ts_cut[threadIdx.x] = tv ? a.cut[t] : 0.0;
    ts_m[threadIdx.x] = tv ? a.mt[t] : 0;
  }
  double2 vx[SH::NV], vy[PB][SH::NV];
  aq_ms_load<T, A16>(a.Xs, n, a.p1, p0, 0, vx);
#pragma unroll
  for (int pb = 0; pb < PB; pb++)
    if (pb < npb) aq_ms_load<T, A16>(a.Yp + (size_t)(b0 + pb) * ystride, n, a.q, q0, 0, vy[pb]);
  for (int i0 = 0; i0 < n; i0 += AQ_MSCREEN_NC) {
    __syncthreads();                             // the panels of the previous chunk have been read
    aq_ms_store<T>(vx, PX);
#pragma unroll
    for (int pb = 0; pb < PB; pb++)
      if (pb < npb) {
        if (MASKED)
          aq_ms_store_masked<T>(vy[pb], PYM + pb * YPAN, PYM + pb * YPAN + PAN);
        else
          aq_ms_store<T>(vy[pb], PYM + pb * YPAN);
      }
    __syncthreads();
    if (i0 + AQ_MSCREEN_NC < n) {
      aq_ms_load<T, A16>(a.Xs, n, a.p1, p0, i0 + AQ_MSCREEN_NC, vx);
#pragma unroll
      for (int pb = 0; pb < PB; pb++)
        if (pb < npb) aq_ms_load<T, A16>(a.Yp + (size_t)(b0 + pb) * ystride, n, a.q, q0, i0 + AQ_MSCREEN_NC, vy[pb]);
    }
#pragma unroll
    for (int kk = 0; kk < AQ_MSCREEN_NC; kk += 4) {
      double x[NI], x2[NI];
#pragma unroll
      for (int i = 0; i < NI; i++) {
        x[i] = px[16 * i * SH::STR + kk];
        if (MASKED) x2[i] = x[i] * x[i];
      }
#pragma unroll
      for (int pb = 0; pb < PB; pb++)
        if (pb < npb) {
          const double *py = PYM + pb * YPAN + yoff;
          double y[NI], m[NI];
#pragma unroll
          for (int i = 0; i < NI; i++) {
            y[i] = py[16 * i * SH::STR + kk];
            if (MASKED) m[i] = py[PAN + 16 * i * SH::STR + kk];
          }
#pragma unroll
          for (int i = 0; i < NI; i++)
#pragma unroll
            for (int jj = 0; jj < NI; jj++) {
              axy[pb][i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[i], x[jj], axy[pb][i][jj], 0, 0, 0);
              if (MASKED) {
                ax[pb][i % NS][jj % NS] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[i], x[jj], ax[pb][i % NS][jj % NS], 0, 0, 0);
                axx[pb][i % NS][jj % NS] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[i], x2[jj], axx[pb][i % NS][jj % NS], 0, 0, 0);
              }
            }
        }
    }
  }

  // ---- epilogue: r^2 of the wave's (T / 2)^2 pairs per permutation, four traits (g + 4 reg) x one predictor (l) per
  // accumulator and lane ----
  double csx[NI], csxx[NI];                        // the complete instance's Sx and Sxx of the lane's predictors
#pragma unroll
  for (int jj = 0; jj < NI; jj++) {
    const int s = p0 + wc * SH::WT + 16 * jj + l;
    csx[jj] = (!MASKED && s < a.p1) ? a.sx[s] : 0.0;
    csxx[jj] = (!MASKED && s < a.p1) ? a.sxx[s] : 0.0;
  }
#pragma unroll
  for (int pb = 0; pb < PB; pb++)
    if (pb < npb) {
      unsigned long long undef = 0;
      unsigned int sel[NI];
#pragma unroll
      for (int jj = 0; jj < NI; jj++) sel[jj] = 0;
#pragma unroll
      for (int i = 0; i < NI; i++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const int tl = wr * SH::WT + 16 * i + g + 4 * reg, t = q0 + tl;
          const bool tv = t < a.q;
          const double syy = ts_syy[tl], cut = ts_cut[tl];
          const int m = ts_m[tl];
          const double md = (double)m;
          const bool t_ok = tv && m - 2 - a.n_cov >= 1 && syy > 0.0;
          double br2 = -1.0;
#pragma unroll
          for (int jj = 0; jj < NI; jj++) {
            const int s = p0 + wc * SH::WT + 16 * jj + l;
            if (tv && s < a.p1) {
              double r = __builtin_nan("");
              bool ok = false;
              if (t_ok) {
                const double sxy = axy[pb][i][jj][reg];
                const double sx = MASKED ? ax[pb][i % NS][jj % NS][reg] : csx[jj];
                const double sxx = MASKED ? axx[pb][i % NS][jj % NS][reg] : csxx[jj];
                const double vx = sxx - sx * sx / md;
                ok = vx > 1e-10 * sxx;
                if (ok) r = sxy / sqrt(vx * syy);
              }
              if (ok) {
                const double r2 = r * r;
                if (r2 >= cut) sel[jj]++;
                if (r2 > br2) br2 = r2;
              } else {
                undef++;
              }
            }
          }
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) {     // across the sixteen predictors of the lane group
            const double o2 = __shfl_xor(br2, off);
            if (o2 > br2) br2 = o2;
          }
          if (l == 0) cmax[wc][pb][tl] = br2;
        }
      const size_t b = (size_t)(b0 + pb);
#pragma unroll
      for (int jj = 0; jj < NI; jj++) {            // the predictor's selected traits over the wave's T / 2 traits
        unsigned int c = sel[jj];
        c += __shfl_xor(c, 16);
        c += __shfl_xor(c, 32);
        const int s = p0 + wc * SH::WT + 16 * jj + l;
        if (g == 0 && c > 0 && s < a.p1) atomicAdd(a.count + b * (size_t)a.p1 + (size_t)s, c);
      }
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) undef += __shfl_xor(undef, off);
      if (lane == 0 && undef > 0) atomicAdd(a.n_undef + b, undef);
    }
  __syncthreads();
  for (int idx = threadIdx.x; idx < PB * T; idx += 256) {   // the two waves of a tile row, then the rows of tiles
    const int pb = idx / T, tl = idx % T;
    if (pb < npb && q0 + tl < a.q) {
      const double m0 = cmax[0][pb][tl], m1 = cmax[1][pb][tl];
      const double m = m1 > m0 ? m1 : m0;
      if (m >= 0.0) atomicMax(a.key + (size_t)(b0 + pb) * (size_t)a.q + (size_t)(q0 + tl), (unsigned long long)__double_as_longlong(m) + 1ull);
    }
  }
}

__global__ __launch_bounds__(256) void aq_k_msperm_reduce(const unsigned int *__restrict__ count, const unsigned long long *__restrict__ key,
                                                         int p1, int q, long long *__restrict__ hs_max, long long *__restrict__ n_sel,
                                                         double *__restrict__ max_r2) {
  __shared__ unsigned long long sh_sum[4];
  __shared__ unsigned int sh_max[4];
  const size_t b = blockIdx.x;
  const unsigned int *row = count + b * (size_t)p1;
  unsigned int mx = 0;
  unsigned long long sum = 0;
  for (int s = threadIdx.x; s < p1; s += 256) {
    const unsigned int c = row[s];
    mx = c > mx ? c : mx;
    sum += c;
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned int om = __shfl_xor(mx, off);
    mx = om > mx ? om : mx;
    sum += __shfl_xor(sum, off);
  }
  if ((threadIdx.x & 63) == 0) {
    sh_sum[threadIdx.x >> 6] = sum;
    sh_max[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; k++) {
      sum += sh_sum[k];
      mx = sh_max[k] > mx ? sh_max[k] : mx;
    }
    hs_max[b] = (long long)mx;
    n_sel[b] = (long long)sum;
  }
  for (int t = threadIdx.x; t < q; t += 256) {
    const unsigned long long k = key[b * (size_t)q + (size_t)t];
    max_r2[b * (size_t)q + (size_t)t] = k ? __longlong_as_double((long long)(k - 1ull)) : -1.0;
  }
}
