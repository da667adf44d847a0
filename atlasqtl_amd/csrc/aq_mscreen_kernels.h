// aq_mscreen_kernels.h -- the marginal screen of a finished prepare handle: the correlation of
// every predictor (column of Xs) with every trait (column of Yc) over the trait's observed rows, on the f64 matrix pipe, and
// what is read off it in registers: the selected pairs, the per-predictor counts, each trait's best predictor.  Included by
// aq_prep_marginal.hip alone; the launch plan is aq_mscreen_plan.h; the tile loop, the pair statistic, the reductions and the
// kernels aq_k_ms_traitstats and aq_k_ms_colstats are those of aq_screen_tile.h.  Every kernel is a plain grid: no workgroup
// waits for another one, nothing spins, and no floating-point atomic is used (the integer atomics are counters), so two calls
// on one handle give the same set of rows and the same bits everywhere else.
//
// The statistic (include/atlasqtl_hip.h, aq_prep_marginal).  For predictor s and trait t, over the m_t observed rows O_t of
// the trait: Sxy = sum x y, Sx = sum x, Sxx = sum x^2, Syy_t = sum y^2; Vx = Sxx - Sx^2 / m_t; r = Sxy / sqrt(Vx Syy_t);
// df_t = m_t - 2 - n_cov.  The pair is undefined (r = NaN, never selected, counted) when Vx <= 1e-10 Sxx, Syy_t = 0 or df_t < 1.
//
// aq_k_ms_tile<T, MASKED, A16>, grid n_tiles, 256 threads.  Workgroup b owns predictors [T tp, T tp + T) x traits
// [T tq, T tq + T), (tp, tq) = (b mod tiles_p, b / tiles_p): the loop of aq_screen_tile.h with one trait-side panel.  Three
// accumulator sets at T = 128 would take 384 registers, so the masked instance exists at T = 64 only (96).  Two workgroups
// share a CU (__launch_bounds__(256, 2): at most 256 registers a lane), so one stages or runs its epilogue while the other
// multiplies.
// Epilogue, in registers: r by aq_ms_pair, the tile's Syy_t, m_t and cutoffs from LDS (read from global memory once per
// workgroup) and the complete instance's Sx, Sxx of the lane's predictors from registers; then
//   - a selected pair (r^2 >= r2_cut[t]) takes a slot from one 64-bit integer counter, which keeps counting beyond cap, and
//     writes (snp, trait, r) there if slot < cap; the order of the rows is unspecified, their set is not;
//   - the per-predictor count of selected traits: summed over the lane's traits, then over the four lane groups, then one
//     integer atomic per predictor and wave;
//   - undefined pairs: counted per wave, one integer atomic;
//   - each trait's best predictor by r^2 within the tile, ties to the lowest predictor index, by the reductions of
//     aq_screen_tile.h, to part[tp][t]; aq_k_ms_best walks tp = 0, 1, ... and takes a later tile only if it is strictly better;
//   - the dense r, if asked for: r_dense[t p1 + s], 16 lanes writing 128 consecutive bytes.
#pragma once
#include "aq_screen_tile.h"   // aq_mscreen_plan.h

struct aq_ms_args {
  const double *Xs, *Yc;              // [p1][n], [q][n]
  int n, p1, q, n_cov, tiles_p;
  const double *sx, *sxx;             // p1 each: the complete instance's Sx and Sxx
  const double *syy;                  // q
  const int *mt;                      // q
  const double *cut;                  // q: the cutoff on r^2
  int32_t *snp, *trait;               // cap rows
  double *r;
  long long cap;
  unsigned long long *n_pairs, *n_undef, *rs;   // two counters; p1 counts
  double *part_r;                     // [tiles_p][q]: r of the tile row's best predictor (NaN: none)
  int32_t *part_s;                    // [tiles_p][q]: that predictor (-1: none)
  double *r_dense;                    // nullptr, or [q][p1]
};

template <int T, bool MASKED, bool A16>
__global__ __launch_bounds__(256, 2) void aq_k_ms_tile(const aq_ms_args a) {
  typedef AqMsShape<T> SH;
  constexpr int NS = MASKED ? SH::NI : 1;
  __shared__ __attribute__((aligned(16))) double PX[SH::PAN];
  __shared__ __attribute__((aligned(16))) double PYM[(MASKED ? 2 : 1) * SH::PAN];
  __shared__ double cand_r[2][T];
  __shared__ int cand_s[2][T];
  __shared__ double ts_syy[T], ts_cut[T];                  // the tile's traits: Syy_t, the cutoff, and m_t (0 for a trait >= q)
  __shared__ int ts_m[T];
  static_assert(sizeof(double) * ((MASKED ? 3 : 2) * SH::PAN) + 2 * T * 12 + T * 20 == aq_mscreen_lds_bytes(T, MASKED), "plan and kernel");
  static_assert(aq_mscreen_lds_bytes(T, MASKED) <= 65536, "64 KB of static LDS");
  const AqMsLane ln;
  const int g = ln.g, l = ln.l, wr = ln.wr, wc = ln.wc;
  const int tp = (int)(blockIdx.x % (unsigned)a.tiles_p), tq = (int)(blockIdx.x / (unsigned)a.tiles_p);
  const int p0 = T * tp, q0 = T * tq;
  if ((int)threadIdx.x < T) {
    aq_ms_trait_fill(ts_syy, a.syy, q0, a.q);
    aq_ms_trait_fill(ts_cut, a.cut, q0, a.q);
    aq_ms_trait_fill(ts_m, a.mt, q0, a.q);
  }
  aq_ms_acc<T, 1> axy;
  aq_ms_acc_m<T, MASKED, 1> ax, axx;
  // one panel, always live (GUARD = NP: nothing tested); its operands are read together with X's
  aq_ms_tile_loop<T, MASKED, A16, 1, 1, AQ_MS_STEP_PAIRED>(a.Xs, a.n, a.p1, p0, a.q, q0, 1, [&](int) { return a.Yc; }, PX, PYM, axy, ax, axx);

  // ---- epilogue: r of the wave's (T / 2)^2 pairs, four traits (g + 4 reg) x one predictor (l) per accumulator and lane ----
  unsigned long long undef = 0;
  unsigned int sel[SH::NI];
  double csx[SH::NI], csxx[SH::NI];
  aq_ms_col_sums<SH::NI, !MASKED>(a.sx, a.sxx, p0 + wc * SH::WT + l, a.p1, csx, csxx);
#pragma unroll
  for (int jj = 0; jj < SH::NI; jj++) sel[jj] = 0;
#pragma unroll
  for (int i = 0; i < SH::NI; i++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int tl = wr * SH::WT + 16 * i + g + 4 * reg, t = q0 + tl;
      const bool tv = t < a.q;
      const double syy = ts_syy[tl], cut = ts_cut[tl];
      const int m = ts_m[tl];
      const double md = (double)m;
      const bool t_ok = tv && m - 2 - a.n_cov >= 1 && syy > 0.0;
      double br2 = -1.0, br = __builtin_nan("");
      int bs = 0x7fffffff;
#pragma unroll
      for (int jj = 0; jj < SH::NI; jj++) {
        const int s = p0 + wc * SH::WT + 16 * jj + l;
        if (tv && s < a.p1) {
          double r = __builtin_nan("");
          const bool ok = t_ok && aq_ms_pair(axy[0][i][jj][reg], MASKED ? ax[0][i % NS][jj % NS][reg] : csx[jj],
                                             MASKED ? axx[0][i % NS][jj % NS][reg] : csxx[jj], md, syy, 0.0, &r);
          if (ok) {
            const double r2 = r * r;
            if (r2 >= cut) {
              sel[jj]++;
              const unsigned long long slot = atomicAdd(a.n_pairs, 1ull);
              if ((long long)slot < a.cap) {
                a.snp[slot] = s;
                a.trait[slot] = t;
                a.r[slot] = r;
              }
            }
            if (r2 > br2) {                        // ascending s: the first of equal r^2 stays
              br2 = r2;
              br = r;
              bs = s;
            }
          } else {
            undef++;
          }
          if (a.r_dense) a.r_dense[(size_t)t * (size_t)a.p1 + (size_t)s] = r;
        }
      }
      aq_ms_lanes_best(br2, br, bs);
      if (l == 0) {
        cand_r[wc][tl] = br;
        cand_s[wc][tl] = bs;
      }
    }
#pragma unroll
  for (int jj = 0; jj < SH::NI; jj++) {            // the predictor's selected traits over the wave's T / 2 traits
    const unsigned int c = aq_ms_lanes_sum(sel[jj], 16, 64);
    const int s = p0 + wc * SH::WT + 16 * jj + l;
    if (g == 0 && c > 0 && s < a.p1) atomicAdd(a.rs + s, (unsigned long long)c);
  }
  undef = aq_ms_lanes_sum(undef, 1, 64);
  if (ln.lane == 0 && undef > 0) atomicAdd(a.n_undef, undef);
  __syncthreads();
  if ((int)threadIdx.x < T && q0 + (int)threadIdx.x < a.q)
    aq_ms_merge_best(cand_r, cand_s, threadIdx.x, a.part_r, a.part_s, (size_t)tp * (size_t)a.q + (size_t)(q0 + (int)threadIdx.x));
}

// each trait's best predictor over the rows of tiles, in the order tp = 0, 1, ...: a later one only if strictly better
static __global__ __launch_bounds__(256) void aq_k_ms_best(const double *__restrict__ part_r, const int32_t *__restrict__ part_s, int tiles_p,
                                                          int q, int32_t *__restrict__ best_snp, double *__restrict__ best_r) {
  const int t = (int)blockIdx.x * 256 + threadIdx.x;
  if (t >= q) return;
  double br = __builtin_nan(""), b2 = -1.0;
  int bs = -1;
  for (int tp = 0; tp < tiles_p; tp++) {
    const int s = part_s[(size_t)tp * q + t];
    const double r = part_r[(size_t)tp * q + t];
    if (s >= 0 && r * r > b2) {
      b2 = r * r;
      br = r;
      bs = s;
    }
  }
  best_snp[t] = bs;
  best_r[t] = br;
}
