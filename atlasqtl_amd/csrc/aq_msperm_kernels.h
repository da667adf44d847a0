// aq_msperm_kernels.h -- permutation nulls of the marginal screen: the statistic of
// aq_mscreen_kernels.h evaluated on (Xs, Y') for permuted responses Y'[i, t] = Yc[perm[b][i], t], many permutations b per
// launch, keeping per permutation only the largest r^2 of every trait, the per-predictor counts of selected traits (on the
// device, reduced there to their maximum and their sum) and the number of undefined pairs.  Nothing of size p1 q exists and no
// pair table is written.  Included by aq_prep_marginal_perm.hip alone; the launch plan is aq_msperm_plan.h; the tile loop, the
// pair statistic, the reductions and the kernels aq_k_ms_gather, aq_k_ms_traitstats and aq_k_ms_colstats are those of
// aq_screen_tile.h.  Every kernel is a plain grid: no workgroup waits for another one, nothing spins, and no floating-point
// atomic is used (the integer atomics are counters and a maximum over bit patterns), so two calls with the same arguments give
// the same bits in every output.
//
// aq_k_ms_gather (NULL order) writes Yp[b][t][i] = Yc[t][perm[b][i]] for the permutations of one launch: Yp has the layout of
// Yc, [q][n] per permutation, so each permutation is one trait-side panel of the tile loop.
//
// aq_k_msperm_tile<T, MASKED, A16, PB>, grid n_tiles groups, 256 threads.  Workgroup w owns the tile v = w mod n_tiles of
// predictors x traits exactly as aq_k_ms_tile owns it, and the permutations PB g ... PB g + PB - 1 of the launch, g = w /
// n_tiles: the loop of aq_screen_tile.h with PB trait-side panels.  Per chunk of 16 samples the panel of X is staged ONCE and
// multiplied against the PB panels of Y': a 64 x 64 tile stages 2 x 64 columns for 64 x 64 outputs; with PB permutations it
// stages (1 + PB) x 64 columns for PB x 64 x 64 outputs, without a second set of X operands.  The identity permutation
// reproduces r of aq_k_ms_tile to the bit.
// Registers (__launch_bounds__(256, 2): 256 a lane).  Accumulators: complete 2 (T / 32)^2 4 PB = 32 PB at T = 64 and 128 PB at
// T = 128; masked 96 PB.  With the staged loads (8 + 8 PB at T = 64) and the operands this admits complete T = 64 with
// PB <= 4, complete T = 128 with PB = 1 and masked (T = 64) with PB <= 2: aq_msperm_instance.  A permutation at or beyond the
// launch's count (the ragged last group) is neither loaded, multiplied nor written; PB = 1 has no such group.
// Epilogue, in registers, per permutation: r^2 by aq_ms_pair; then
//   - the largest defined r^2 of a trait, by the reductions of aq_screen_tile.h, into ONE integer atomicMax per (permutation,
//     trait) and workgroup;
//   - the per-(permutation, predictor) count of selected traits: summed over the lane's traits, over the four lane groups,
//     then one integer atomic per predictor and wave where it is not zero;
//   - undefined pairs: counted per wave, one integer atomic per permutation.
//
// aq_k_msperm_reduce, grid = the launch's permutations, 256 threads: count[b][.] -> hs_max[b] (the largest) and n_sel[b] (the
// sum), integers added in a fixed order; key -> max_r2[b][t], -1.0 where the key is 0.
#pragma once
#include "aq_msperm_plan.h"
#include "aq_screen_tile.h"

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

template <int T, bool MASKED, bool A16, int PB>
__global__ __launch_bounds__(256, 2) void aq_k_msperm_tile(const aq_msp_args a) {
  typedef AqMsShape<T> SH;
  static_assert(aq_msperm_instance(T, MASKED, PB), "an instance of the plan");
  constexpr int NI = SH::NI;
  constexpr int NS = MASKED ? NI : 1;
  constexpr int YPAN = (MASKED ? 2 : 1) * SH::PAN;         // per permutation: PY, then (MASKED) PM
  __shared__ __attribute__((aligned(16))) double PX[SH::PAN];
  __shared__ __attribute__((aligned(16))) double PYM[PB * YPAN];
  __shared__ double ts_syy[T], ts_cut[T];                  // the tile's traits: Syy_t, the cutoff, and m_t (0 for a trait >= q)
  __shared__ int ts_m[T];
  __shared__ double cmax[2][PB][T];                        // per wave column: a trait's largest r^2 (-1.0: none)
  static_assert(sizeof(double) * (SH::PAN + PB * YPAN) + T * 20 + sizeof(double) * 2 * PB * T == aq_msperm_lds_bytes(T, MASKED, PB),
                "plan and kernel");
  static_assert(aq_msperm_lds_bytes(T, MASKED, PB) <= 65536, "64 KB of static LDS");
  const AqMsLane ln;
  const int g = ln.g, l = ln.l, wr = ln.wr, wc = ln.wc;
  const int v = (int)(blockIdx.x % (unsigned)a.n_tiles), grp = (int)(blockIdx.x / (unsigned)a.n_tiles);
  const int tp = v % a.tiles_p, tq = v / a.tiles_p;
  const int p0 = T * tp, q0 = T * tq;
  const int b0 = PB * grp;
  const int npb = a.nb - b0 < PB ? a.nb - b0 : PB;         // the group's permutations: >= 1 by the grid
  const size_t ystride = (size_t)a.q * (size_t)a.n;
  if ((int)threadIdx.x < T) {
    aq_ms_trait_fill(ts_syy, a.syy, q0, a.q);
    aq_ms_trait_fill(ts_cut, a.cut, q0, a.q);
    aq_ms_trait_fill(ts_m, a.mt, q0, a.q);
  }
  aq_ms_acc<T, PB> axy;
  aq_ms_acc_m<T, MASKED, PB> ax, axx;
  // PB > 1: every panel is tested against npb (GUARD = 0, the ragged last group).  PB = 1: the one panel is live (GUARD = NP)
  // and the chunk's four steps are kept apart, which holds the kernel to its 76-78 registers
  aq_ms_tile_loop<T, MASKED, A16, PB, (PB > 1 ? 0 : 1), (PB == 1 ? AQ_MS_STEP_FENCED : AQ_MS_STEP_PLAIN)>(a.Xs, a.n, a.p1, p0, a.q, q0, npb,
                                                [&](int pb) { return a.Yp + (size_t)(b0 + pb) * ystride; }, PX, PYM, axy, ax, axx);

  // ---- epilogue: r^2 of the wave's (T / 2)^2 pairs per permutation, four traits (g + 4 reg) x one predictor (l) per
  // accumulator and lane ----
  double csx[NI], csxx[NI];
  aq_ms_col_sums<NI, !MASKED>(a.sx, a.sxx, p0 + wc * SH::WT + l, a.p1, csx, csxx);
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
              const bool ok = t_ok && aq_ms_pair(axy[pb][i][jj][reg], MASKED ? ax[pb][i % NS][jj % NS][reg] : csx[jj],
                                                 MASKED ? axx[pb][i % NS][jj % NS][reg] : csxx[jj], md, syy, 0.0, &r);
              if (ok) {
                const double r2 = r * r;
                if (r2 >= cut) sel[jj]++;
                if (r2 > br2) br2 = r2;
              } else {
                undef++;
              }
            }
          }
          br2 = aq_ms_lanes_max(br2);
          if (l == 0) cmax[wc][pb][tl] = br2;
        }
      const size_t b = (size_t)(b0 + pb);
#pragma unroll
      for (int jj = 0; jj < NI; jj++) {            // the predictor's selected traits over the wave's T / 2 traits
        const unsigned int c = aq_ms_lanes_sum(sel[jj], 16, 64);
        const int s = p0 + wc * SH::WT + 16 * jj + l;
        if (g == 0 && c > 0 && s < a.p1) atomicAdd(a.count + b * (size_t)a.p1 + (size_t)s, c);
      }
      undef = aq_ms_lanes_sum(undef, 1, 64);
      if (ln.lane == 0 && undef > 0) atomicAdd(a.n_undef + b, undef);
    }
  __syncthreads();
  for (int idx = threadIdx.x; idx < PB * T; idx += 256) {   // the two waves of a tile row, then the rows of tiles
    const int pb = idx / T, tl = idx % T;
    if (pb < npb && q0 + tl < a.q)
      aq_ms_key_max(cmax[0][pb][tl], cmax[1][pb][tl], a.key + (size_t)(b0 + pb) * (size_t)a.q + (size_t)(q0 + tl));
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
  for (int t = threadIdx.x; t < q; t += 256) max_r2[b * (size_t)q + (size_t)t] = aq_ms_key_r2(key[b * (size_t)q + (size_t)t]);
}
