// aq_cis_kernels.h -- the cis scan of a finished prepare handle: the statistic of aq_mscreen_kernels.h
// evaluated only for the pairs (predictor s, trait t) with s_lo[t] <= s < s_hi[t], a band of the p1 x q matrix, and the
// permutation null of each trait's best in-window predictor.  Included through aq_cis_host.h by aq_prep_cis.hip,
// aq_prep_cis_cond.hip and aq_prep_cis_int.hip, so its kernels that are no templates are static; the launch plan, the order of the traits and the list
// of work items are aq_cis_plan.h; the tile loop, the pair statistic, the reductions and the kernels aq_k_ms_gather,
// aq_k_ms_traitstats and aq_k_ms_colstats are those of aq_screen_tile.h.  Every kernel is a plain grid: no workgroup waits for
// another one, nothing spins, and no floating-point atomic is used (the integer atomics are counters and a maximum over bit
// patterns), so two calls give the same set of rows and the same bits everywhere else.
//
// aq_k_ms_gather writes Yp[b][j][i] = Yc[order[j]][perm[b][i]] for the q_active ordered traits with a window and the
// permutations of one launch; without perm (the scan) it is the ordered copy Yo[j][i] = Yc[order[j]][i].  With the traits of
// a tile contiguous, [q_active][n], each is one trait-side panel of the tile loop.
//
// aq_k_cis_tile<MASKED, A16>, grid W, 256 threads.  Work item w = (k, p0) = (item_tile[w], item_p0[w]): predictors
// [p0, p0 + 64) against the ordered traits [64 k, 64 k + 64), by the loop of aq_screen_tile.h with one trait-side panel, so r
// of a pair is r of the plain screen to the bit.  Per trait of the tile Syy_t, the cutoff, m_t, s_lo, s_hi and the trait's own
// index are read into LDS once.  Epilogue (aq_cis_scan_epilogue, which the conditional scan shares), in registers: a pair
// exists iff s_lo <= s < s_hi (s_hi <= p1); for a pair that exists r and ok by aq_ms_pair, then
//   - a selected pair (r^2 >= cut) takes a slot from one 64-bit integer counter, which keeps counting beyond cap, and writes
//     (snp, the trait's own index, r) there if slot < cap;
//   - undefined pairs: per trait, summed over the sixteen lanes of a lane group, one integer atomic where it is not zero;
//   - the item's best predictor of each trait, ties to the lowest index, by the reductions of aq_screen_tile.h, into
//     part[w][64].
// aq_k_cis_best, one thread per ordered trait: its tile's items in ascending p0, a later one only if strictly better; the
// result under the trait's own index, -1 / NaN for a trait without a defined pair or without a window.
//
// aq_k_cis_perm_tile<MASKED, A16, PB>, grid W groups, groups = ceil(nb / PB).  Workgroup w owns the item w mod W and the
// permutations PB g ... PB g + PB - 1, g = w / W: the loop with PB trait-side panels, as in aq_k_msperm_tile<64, MASKED, A16,
// PB>, whose registers (32 PB accumulator registers complete, 96 PB masked) and LDS it has.  A permutation at or beyond nb
// (the ragged last group) is neither loaded, multiplied nor written.  Its epilogue keeps only the largest in-window r^2 per
// (permutation, trait), into ONE integer atomicMax per (permutation, trait) and workgroup.
// aq_k_cis_reduce: key -> max_r2[b][t], -1.0 where the key is 0.
#pragma once
#include "aq_cis_plan.h"
#include "aq_screen_tile.h"

struct aq_cis_args {
  const double *Xs, *Yo;              // [p1][n]; [q_active][n] (the scan) or [nb][q_active][n] (permutations)
  int n, p1, q, qa, n_cov, W, nb;     // qa: the ordered traits with a window; nb: the permutations of this launch
  const int32_t *item_tile, *item_p0; // W each
  const double *sx, *sxx;             // p1 each: the complete instances' Sx and Sxx
  // per ordered trait j < qa
  const double *syy, *cut;
  const int *mt;
  const int32_t *lo, *hi, *orig;      // the window and the trait's own index
  // the scan
  int32_t *snp, *trait;               // cap rows
  double *r;
  long long cap;
  unsigned long long *n_pairs, *n_undef;   // one counter; q counts under the trait's own index
  double *part_r;                     // [W][64]: r of the item's best predictor (NaN: none)
  int32_t *part_s;                    // [W][64]: that predictor (-1: none)
  // the permutations
  unsigned long long *key;            // [nb][q]: bits(max r^2) + 1, 0: no defined pair
};

// the per-trait arrays of a work item that every cis tile kernel holds in LDS: an empty window for a trait >= qa
struct AqCisWin {
  int lo[AQ_CIS_TILE], hi[AQ_CIS_TILE], orig[AQ_CIS_TILE];
  __device__ __forceinline__ void fill(const aq_cis_args &a, int q0) {   // threadIdx.x < AQ_CIS_TILE
    aq_ms_trait_fill(lo, a.lo, q0, a.qa);
    aq_ms_trait_fill(hi, a.hi, q0, a.qa);
    aq_ms_trait_fill(orig, a.orig, q0, a.qa);
  }
};

// what the statistic needs of a trait: whether it can be tested at all, Syy_t (or S~yy_t) and m_t as a double
struct AqCisTrait {
  bool ok;
  double syy, m;
};

// The epilogue of a scan over work item (p0, q0) of workgroup blockIdx.x: four traits (g + 4 reg) x one predictor (l) per
// accumulator and lane.  trait(tl): the AqCisTrait of trait tl of the tile, read once per trait; stat(i, jj, reg, tr, &r):
// whether the pair of accumulator (i, jj), register reg is defined for a testable trait tr, and then its r.
template <typename Trait, typename Stat>
__device__ __forceinline__ void aq_cis_scan_epilogue(const aq_cis_args &a, int p0, int q0, const double (&ts_cut)[AQ_CIS_TILE], const AqCisWin &win,
                                                     double (&cand_r)[2][AQ_CIS_TILE], int (&cand_s)[2][AQ_CIS_TILE], Trait trait, Stat stat) {
  constexpr int T = AQ_CIS_TILE;
  typedef AqMsShape<T> SH;
  const AqMsLane ln;
  const int g = ln.g, l = ln.l, wr = ln.wr, wc = ln.wc;
#pragma unroll
  for (int i = 0; i < SH::NI; i++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int tl = wr * SH::WT + 16 * i + g + 4 * reg;
      const double cut = ts_cut[tl];
      const int lo = win.lo[tl], hi = win.hi[tl], t = win.orig[tl];
      const AqCisTrait tr = trait(tl);
      double br2 = -1.0, br = __builtin_nan("");
      int bs = 0x7fffffff;
      unsigned int undef = 0;
#pragma unroll
      for (int jj = 0; jj < SH::NI; jj++) {
        const int s = p0 + wc * SH::WT + 16 * jj + l;
        if (s >= lo && s < hi) {                   // hi <= p1, and lo = hi = 0 for a trait >= qa: the pair exists
          double r = __builtin_nan("");
          if (tr.ok && stat(i, jj, reg, tr, &r)) {
            const double r2 = r * r;
            if (r2 >= cut) {
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
        }
      }
      aq_ms_lanes_best(br2, br, bs);
      undef = aq_ms_lanes_sum(undef, 1, 16);
      if (l == 0) {
        cand_r[wc][tl] = br;
        cand_s[wc][tl] = bs;
        if (undef > 0) atomicAdd(a.n_undef + t, (unsigned long long)undef);   // undef > 0: a pair exists, so the trait is one < qa
      }
    }
  __syncthreads();
  if ((int)threadIdx.x < T && q0 + (int)threadIdx.x < a.qa)
    aq_ms_merge_best(cand_r, cand_s, threadIdx.x, a.part_r, a.part_s, (size_t)blockIdx.x * (size_t)T + (size_t)threadIdx.x);
}

template <bool MASKED, bool A16>
__global__ __launch_bounds__(256, 2) void aq_k_cis_tile(const aq_cis_args a) {
  constexpr int T = AQ_CIS_TILE;
  typedef AqMsShape<T> SH;
  constexpr int NS = MASKED ? SH::NI : 1;
  __shared__ __attribute__((aligned(16))) double PX[SH::PAN];
  __shared__ __attribute__((aligned(16))) double PYM[(MASKED ? 2 : 1) * SH::PAN];
  __shared__ double cand_r[2][T];
  __shared__ int cand_s[2][T];
  __shared__ double ts_syy[T], ts_cut[T];                  // the tile's traits; m_t = 0 for a trait >= qa
  __shared__ int ts_m[T];
  __shared__ AqCisWin win;
  static_assert(sizeof(double) * ((MASKED ? 3 : 2) * SH::PAN) + 2 * T * 12 + T * 32 == aq_cis_lds_bytes(MASKED), "plan and kernel");
  static_assert(sizeof(AqCisWin) == T * 12 && aq_cis_lds_bytes(MASKED) <= 65536, "64 KB of static LDS");
  const AqMsLane ln;
  const int p0 = a.item_p0[blockIdx.x], q0 = T * a.item_tile[blockIdx.x];
  if ((int)threadIdx.x < T) {
    aq_ms_trait_fill(ts_syy, a.syy, q0, a.qa);
    aq_ms_trait_fill(ts_cut, a.cut, q0, a.qa);
    aq_ms_trait_fill(ts_m, a.mt, q0, a.qa);
    win.fill(a, q0);
  }
  aq_ms_acc<T, 1> axy;
  aq_ms_acc_m<T, MASKED, 1> ax, axx;
  // one panel, always live (GUARD = NP: nothing tested); its operands are read together with X's
  aq_ms_tile_loop<T, MASKED, A16, 1, 1, AQ_MS_STEP_PAIRED>(a.Xs, a.n, a.p1, p0, a.qa, q0, 1, [&](int) { return a.Yo; }, PX, PYM, axy, ax, axx);
  double csx[SH::NI], csxx[SH::NI];
  aq_ms_col_sums<SH::NI, !MASKED>(a.sx, a.sxx, p0 + ln.wc * SH::WT + ln.l, a.p1, csx, csxx);
  aq_cis_scan_epilogue(
      a, p0, q0, ts_cut, win, cand_r, cand_s,
      [&](int tl) { return AqCisTrait{ts_m[tl] - 2 - a.n_cov >= 1 && ts_syy[tl] > 0.0, ts_syy[tl], (double)ts_m[tl]}; },
      [&](int i, int jj, int reg, const AqCisTrait &tr, double *r) {
        return aq_ms_pair(axy[0][i][jj][reg], MASKED ? ax[0][i % NS][jj % NS][reg] : csx[jj],
                          MASKED ? axx[0][i % NS][jj % NS][reg] : csxx[jj], tr.m, tr.syy, 0.0, r);
      });
}

// each trait's best predictor over its tile's items, in ascending p0: a later one only if strictly better.  One thread per
// position j of the order: j >= qa is a trait without a window.
static __global__ __launch_bounds__(256) void aq_k_cis_best(const double *__restrict__ part_r, const int32_t *__restrict__ part_s,
                                                           const int32_t *__restrict__ first_item, const int32_t *__restrict__ order,
                                                           int qa, int q, int32_t *__restrict__ best_snp, double *__restrict__ best_r) {
  const int j = (int)blockIdx.x * 256 + threadIdx.x;
  if (j >= q) return;
  double br = __builtin_nan(""), b2 = -1.0;
  int bs = -1;
  if (j < qa) {
    const int k = j / AQ_CIS_TILE, tl = j % AQ_CIS_TILE;
    for (int w = first_item[k]; w < first_item[k + 1]; w++) {
      const int s = part_s[(size_t)w * AQ_CIS_TILE + tl];
      const double r = part_r[(size_t)w * AQ_CIS_TILE + tl];
      if (s >= 0 && r * r > b2) {
        b2 = r * r;
        br = r;
        bs = s;
      }
    }
  }
  best_snp[order[j]] = bs;
  best_r[order[j]] = br;
}

template <bool MASKED, bool A16, int PB>
__global__ __launch_bounds__(256, 2) void aq_k_cis_perm_tile(const aq_cis_args a) {
  constexpr int T = AQ_CIS_TILE;
  typedef AqMsShape<T> SH;
  static_assert(aq_cis_instance(MASKED, PB), "an instance of the plan");
  constexpr int NI = SH::NI;
  constexpr int NS = MASKED ? NI : 1;
  constexpr int YPAN = (MASKED ? 2 : 1) * SH::PAN;         // per permutation: PY, then (MASKED) PM
  __shared__ __attribute__((aligned(16))) double PX[SH::PAN];
  __shared__ __attribute__((aligned(16))) double PYM[PB * YPAN];
  __shared__ double ts_syy[T];                             // the tile's traits; m_t = 0 for a trait >= qa
  __shared__ int ts_m[T];
  __shared__ AqCisWin win;
  __shared__ double cmax[2][PB][T];                        // per wave column: a trait's largest r^2 (-1.0: none)
  static_assert(sizeof(double) * (SH::PAN + PB * YPAN) + T * 24 + sizeof(double) * 2 * PB * T == aq_cis_perm_lds_bytes(MASKED, PB),
                "plan and kernel");
  static_assert(sizeof(AqCisWin) == T * 12 && aq_cis_perm_lds_bytes(MASKED, PB) <= 65536, "64 KB of static LDS");
  const AqMsLane ln;
  const int g = ln.g, l = ln.l, wr = ln.wr, wc = ln.wc;
  const int v = (int)(blockIdx.x % (unsigned)a.W), grp = (int)(blockIdx.x / (unsigned)a.W);
  const int p0 = a.item_p0[v], q0 = T * a.item_tile[v];
  const int b0 = PB * grp;
  const int npb = a.nb - b0 < PB ? a.nb - b0 : PB;         // the group's permutations: >= 1 by the grid
  const size_t ystride = (size_t)a.qa * (size_t)a.n;
  if ((int)threadIdx.x < T) {
    aq_ms_trait_fill(ts_syy, a.syy, q0, a.qa);
    aq_ms_trait_fill(ts_m, a.mt, q0, a.qa);
    win.fill(a, q0);
  }
  aq_ms_acc<T, PB> axy;
  aq_ms_acc_m<T, MASKED, PB> ax, axx;
  // PB > 1: every panel is tested against npb (GUARD = 0, the ragged last group).  PB = 1: the one panel is live (GUARD = NP)
  // and the chunk's four steps are kept apart, which holds the kernel to its 76-78 registers
  aq_ms_tile_loop<T, MASKED, A16, PB, (PB > 1 ? 0 : 1), (PB == 1 ? AQ_MS_STEP_FENCED : AQ_MS_STEP_PLAIN)>(a.Xs, a.n, a.p1, p0, a.qa, q0, npb,
                                                [&](int pb) { return a.Yo + (size_t)(b0 + pb) * ystride; }, PX, PYM, axy, ax, axx);

  // ---- epilogue: the largest in-window r^2 per permutation and trait ----
  double csx[NI], csxx[NI];
  aq_ms_col_sums<NI, !MASKED>(a.sx, a.sxx, p0 + wc * SH::WT + l, a.p1, csx, csxx);
#pragma unroll
  for (int pb = 0; pb < PB; pb++)
    if (pb < npb) {
#pragma unroll
      for (int i = 0; i < NI; i++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const int tl = wr * SH::WT + 16 * i + g + 4 * reg;
          const double syy = ts_syy[tl];
          const int m = ts_m[tl], lo = win.lo[tl], hi = win.hi[tl];
          const double md = (double)m;
          const bool t_ok = m - 2 - a.n_cov >= 1 && syy > 0.0;
          double br2 = -1.0;
#pragma unroll
          for (int jj = 0; jj < NI; jj++) {
            const int s = p0 + wc * SH::WT + 16 * jj + l;
            double r;
            if (t_ok && s >= lo && s < hi &&
                aq_ms_pair(axy[pb][i][jj][reg], MASKED ? ax[pb][i % NS][jj % NS][reg] : csx[jj],
                           MASKED ? axx[pb][i % NS][jj % NS][reg] : csxx[jj], md, syy, 0.0, &r)) {
              const double r2 = r * r;
              if (r2 > br2) br2 = r2;
            }
          }
          br2 = aq_ms_lanes_max(br2);
          if (l == 0) cmax[wc][pb][tl] = br2;
        }
    }
  __syncthreads();
  for (int idx = threadIdx.x; idx < PB * T; idx += 256) {   // the two waves of a tile row, then the items of the trait tile
    const int pb = idx / T, tl = idx % T;
    if (pb < npb && q0 + tl < a.qa)
      aq_ms_key_max(cmax[0][pb][tl], cmax[1][pb][tl], a.key + (size_t)(b0 + pb) * (size_t)a.q + (size_t)win.orig[tl]);
  }
}

static __global__ __launch_bounds__(256) void aq_k_cis_reduce(const unsigned long long *__restrict__ key, long long count,
                                                             double *__restrict__ max_r2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) max_r2[i] = aq_ms_key_r2(key[i]);
}
