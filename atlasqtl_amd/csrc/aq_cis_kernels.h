// aq_cis_kernels.h -- the cis scan of a finished prepare handle: the statistic of aq_mscreen_kernels.h
// evaluated only for the pairs (predictor s, trait t) with s_lo[t] <= s < s_hi[t], a band of the p1 x q matrix, and the
// permutation null of each trait's best in-window predictor.  Included by aq_prep_cis.hip alone; the launch plan, the order of
// the traits and the list of work items are aq_cis_plan.h.  Every kernel is a plain grid: no workgroup waits for another one,
// nothing spins, and no floating-point atomic is used (the integer atomics are counters and a maximum over bit patterns), so
// two calls give the same set of rows and the same bits everywhere else.
//
// aq_k_cis_gather: Yp[b][j][i] = Yc[order[j]][perm[b][i]] for the q_active ordered traits with a window and the permutations
// of one launch; without perm (the scan) it is the ordered copy Yo[j][i] = Yc[order[j]][i].  A workgroup writes whole columns,
// 256 consecutive doubles at a time (coalesced); its scattered reads stay inside one column of Yc.  NaN moves with the value.
// The host has checked every index of perm and built order.  With the traits of a tile contiguous, [q_active][n], the tile
// loops keep the 16-byte loads, the LDS rows of 18 doubles and the bank argument of aq_k_ms_tile<64, ...> and use its
// aq_ms_load, aq_ms_store and aq_ms_store_masked.
//
// aq_k_cis_tile<MASKED, A16>, grid W, 256 threads.  Work item w = (k, p0) = (item_tile[w], item_p0[w]): predictors
// [p0, p0 + 64) against the ordered traits [64 k, 64 k + 64).  The loop body is that of aq_k_ms_tile<64, MASKED, A16>: every
// output element is accumulated over the samples in its order, one MFMA per step of 4, so r of a pair is r of the plain
// screen to the bit.  Per trait of the tile Syy_t, the cutoff, m_t, s_lo, s_hi and the trait's own index are read into LDS
// once, before the loop.  Epilogue, in registers: a pair exists iff s_lo <= s < s_hi (s_hi <= p1); for a pair that exists r
// and ok by the expression of aq_k_ms_tile, then
//   - a selected pair (r^2 >= cut) takes a slot from one 64-bit integer counter, which keeps counting beyond cap, and writes
//     (snp, the trait's own index, r) there if slot < cap;
//   - undefined pairs: per trait, summed over the sixteen lanes of a lane group, one integer atomic where it is not zero;
//   - the item's best predictor of each trait, ties to the lowest index, by the route of aq_k_ms_tile, into part[w][64].
// aq_k_cis_best, one thread per ordered trait: its tile's items in ascending p0, a later one only if strictly better; the
// result under the trait's own index, -1 / NaN for a trait without a defined pair or without a window.
//
// aq_k_cis_perm_tile<MASKED, A16, PB>, grid W groups, groups = ceil(nb / PB).  Workgroup w owns the item w mod W and the
// permutations PB g ... PB g + PB - 1, g = w / W: the panel of X is staged ONCE per chunk and multiplied against the PB panels
// of Y', as in aq_k_msperm_tile<64, MASKED, A16, PB>, whose registers (32 PB accumulator registers complete, 96 PB masked)
// and LDS it has.  A permutation at or beyond nb (the ragged last group) is neither loaded, multiplied nor written.  Its
// epilogue keeps only the largest in-window r^2 per (permutation, trait): over the lane's predictors, the sixteen lanes, the
// two waves of a tile row through LDS, then ONE integer atomicMax per (permutation, trait) and workgroup on key = bits(r^2) + 1
// (r^2 >= 0: the order of the bit patterns is the order of the values; key 0: none).
// aq_k_cis_reduce: key -> max_r2[b][t], -1.0 where the key is 0.
#pragma once
#include "aq_cis_plan.h"
#include "aq_mscreen_kernels.h"   // aq_ms_d4, AqMsShape, aq_ms_load, aq_ms_store, aq_ms_store_masked

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

static __global__ __launch_bounds__(256) void aq_k_cis_gather(const double *__restrict__ Yc, const int32_t *__restrict__ order,
                                                             const int32_t *__restrict__ perm, int n, int qa, int nb,
                                                             double *__restrict__ Yp) {
  const long long cols = (long long)nb * (long long)qa;
  for (long long c = blockIdx.x; c < cols; c += gridDim.x) {
    const double *src = Yc + (size_t)order[c % qa] * (size_t)n;
    double *dst = Yp + (size_t)c * (size_t)n;
    if (perm) {
      const int32_t *row = perm + (size_t)(c / qa) * (size_t)n;
      for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[row[i]];
    } else {
      for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
    }
  }
}

template <bool MASKED, bool A16>
__global__ __launch_bounds__(256, 2) void aq_k_cis_tile(const aq_cis_args a) {
  constexpr int T = AQ_CIS_TILE;
  typedef AqMsShape<T> SH;
  constexpr int NS = MASKED ? SH::NI : 1;                  // extent of the two extra accumulator sets (1: unused)
  __shared__ __attribute__((aligned(16))) double PX[T * SH::STR];
  __shared__ __attribute__((aligned(16))) double PYM[(MASKED ? 2 : 1) * T * SH::STR];
  double *const PY = PYM, *const PM = PYM + (MASKED ? T * SH::STR : 0);   // PM is read and written by the masked instance only
  __shared__ double cand_r[2][T];
  __shared__ int cand_s[2][T];
  __shared__ double ts_syy[T], ts_cut[T];                  // the tile's traits; m_t = 0 and an empty window for a trait >= qa
  __shared__ int ts_m[T], ts_lo[T], ts_hi[T], ts_orig[T];
  static_assert(sizeof(double) * ((MASKED ? 3 : 2) * T * SH::STR) + 2 * T * 12 + T * 32 == aq_cis_lds_bytes(MASKED), "plan and kernel");
  static_assert(aq_cis_lds_bytes(MASKED) <= 65536, "64 KB of static LDS");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, l = lane & 15;
  const int wr = w >> 1, wc = w & 1;
  const int p0 = a.item_p0[blockIdx.x], q0 = T * a.item_tile[blockIdx.x];
  const int n = a.n;
  aq_ms_d4 axy[SH::NI][SH::NI], ax[NS][NS], axx[NS][NS];
#pragma unroll
  for (int i = 0; i < SH::NI; i++)
#pragma unroll
    for (int jj = 0; jj < SH::NI; jj++) axy[i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < NS; i++)
#pragma unroll
    for (int jj = 0; jj < NS; jj++) {
      ax[i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
      axx[i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
    }
  const double *py = PY + (wr * SH::WT + l) * SH::STR + g;
  const double *pm = PM + (wr * SH::WT + l) * SH::STR + g;
  const double *px = PX + (wc * SH::WT + l) * SH::STR + g;
  if ((int)threadIdx.x < T) {                      // read after the loop's barriers
    const int j = q0 + (int)threadIdx.x;
    const bool tv = j < a.qa;
    ts_syy[threadIdx.x] = tv ? a.syy[j] : 0.0;
    ts_cut[threadIdx.x] = tv ? a.cut[j] : 0.0;
    ts_m[threadIdx.x] = tv ? a.mt[j] : 0;
    ts_lo[threadIdx.x] = tv ? a.lo[j] : 0;
    ts_hi[threadIdx.x] = tv ? a.hi[j] : 0;
    ts_orig[threadIdx.x] = tv ? a.orig[j] : 0;
  }
  double2 vx[SH::NV], vy[SH::NV];
  aq_ms_load<T, A16>(a.Xs, n, a.p1, p0, 0, vx);
  aq_ms_load<T, A16>(a.Yo, n, a.qa, q0, 0, vy);
  for (int i0 = 0; i0 < n; i0 += AQ_MSCREEN_NC) {
    __syncthreads();                             // the panels of the previous chunk have been read
    aq_ms_store<T>(vx, PX);
    if (MASKED)
      aq_ms_store_masked<T>(vy, PY, PM);
    else
      aq_ms_store<T>(vy, PY);
    __syncthreads();
    if (i0 + AQ_MSCREEN_NC < n) {
      aq_ms_load<T, A16>(a.Xs, n, a.p1, p0, i0 + AQ_MSCREEN_NC, vx);
      aq_ms_load<T, A16>(a.Yo, n, a.qa, q0, i0 + AQ_MSCREEN_NC, vy);
    }
#pragma unroll
    for (int kk = 0; kk < AQ_MSCREEN_NC; kk += 4) {
      double y[SH::NI], m[SH::NI], x[SH::NI], x2[SH::NI];
#pragma unroll
      for (int i = 0; i < SH::NI; i++) {
        y[i] = py[16 * i * SH::STR + kk];
        x[i] = px[16 * i * SH::STR + kk];
        if (MASKED) {
          m[i] = pm[16 * i * SH::STR + kk];
          x2[i] = x[i] * x[i];
        }
      }
#pragma unroll
      for (int i = 0; i < SH::NI; i++)
#pragma unroll
        for (int jj = 0; jj < SH::NI; jj++) {
          axy[i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[i], x[jj], axy[i][jj], 0, 0, 0);
          if (MASKED) {
            ax[i % NS][jj % NS] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[i], x[jj], ax[i % NS][jj % NS], 0, 0, 0);
            axx[i % NS][jj % NS] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[i], x2[jj], axx[i % NS][jj % NS], 0, 0, 0);
          }
        }
    }
  }

  // ---- epilogue: r of the wave's 32 x 32 pairs, four traits (g + 4 reg) x one predictor (l) per accumulator and lane ----
  double csx[SH::NI], csxx[SH::NI];                // the complete instance's Sx and Sxx of the lane's predictors
#pragma unroll
  for (int jj = 0; jj < SH::NI; jj++) {
    const int s = p0 + wc * SH::WT + 16 * jj + l;
    csx[jj] = (!MASKED && s < a.p1) ? a.sx[s] : 0.0;
    csxx[jj] = (!MASKED && s < a.p1) ? a.sxx[s] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < SH::NI; i++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int tl = wr * SH::WT + 16 * i + g + 4 * reg;
      const double syy = ts_syy[tl], cut = ts_cut[tl];
      const int m = ts_m[tl], lo = ts_lo[tl], hi = ts_hi[tl], t = ts_orig[tl];
      const double md = (double)m;
      const bool t_ok = m - 2 - a.n_cov >= 1 && syy > 0.0;
      double br2 = -1.0, br = __builtin_nan("");
      int bs = 0x7fffffff;
      unsigned int undef = 0;
#pragma unroll
      for (int jj = 0; jj < SH::NI; jj++) {
        const int s = p0 + wc * SH::WT + 16 * jj + l;
        if (s >= lo && s < hi) {                   // hi <= p1, and lo = hi = 0 for a trait >= qa: the pair exists
          double r = __builtin_nan("");
          bool ok = false;
          if (t_ok) {
            const double sxy = axy[i][jj][reg];
            const double sx = MASKED ? ax[i % NS][jj % NS][reg] : csx[jj];
            const double sxx = MASKED ? axx[i % NS][jj % NS][reg] : csxx[jj];
            const double vx = sxx - sx * sx / md;
            ok = vx > 1e-10 * sxx;
            if (ok) r = sxy / sqrt(vx * syy);
          }
          if (ok) {
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
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {     // across the sixteen predictors of the lane group
        const double o2 = __shfl_xor(br2, off), orr = __shfl_xor(br, off);
        const int os = __shfl_xor(bs, off);
        undef += __shfl_xor(undef, off);
        if (o2 > br2 || (o2 == br2 && os < bs)) {
          br2 = o2;
          br = orr;
          bs = os;
        }
      }
      if (l == 0) {
        cand_r[wc][tl] = br;
        cand_s[wc][tl] = bs;
        if (undef > 0) atomicAdd(a.n_undef + t, (unsigned long long)undef);   // undef > 0: a pair exists, so the trait is one < qa
      }
    }
  __syncthreads();
  if ((int)threadIdx.x < T && q0 + (int)threadIdx.x < a.qa) {   // the two waves of a tile row: the lower predictors win a tie
    const int tl = threadIdx.x;
    double r = cand_r[0][tl];
    int s = cand_s[0][tl];
    const double r1 = cand_r[1][tl];
    const int s1 = cand_s[1][tl];
    if (s1 != 0x7fffffff && (s == 0x7fffffff || r1 * r1 > r * r)) {
      r = r1;
      s = s1;
    }
    const size_t o = (size_t)blockIdx.x * (size_t)T + (size_t)tl;
    a.part_r[o] = r;
    a.part_s[o] = s == 0x7fffffff ? -1 : s;
  }
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
  constexpr int NS = MASKED ? NI : 1;                      // extent of the two extra accumulator sets (1: unused)
  constexpr int PAN = T * SH::STR;                         // doubles of a panel
  constexpr int YPAN = (MASKED ? 2 : 1) * PAN;             // per permutation: PY, then (MASKED) PM
  __shared__ __attribute__((aligned(16))) double PX[PAN];
  __shared__ __attribute__((aligned(16))) double PYM[PB * YPAN];
  __shared__ double ts_syy[T];                             // the tile's traits; m_t = 0 and an empty window for a trait >= qa
  __shared__ int ts_m[T], ts_lo[T], ts_hi[T], ts_orig[T];
  __shared__ double cmax[2][PB][T];                        // per wave column: a trait's largest r^2 (-1.0: none)
  static_assert(sizeof(double) * (PAN + PB * YPAN) + T * 24 + sizeof(double) * 2 * PB * T == aq_cis_perm_lds_bytes(MASKED, PB),
                "plan and kernel");
  static_assert(aq_cis_perm_lds_bytes(MASKED, PB) <= 65536, "64 KB of static LDS");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, l = lane & 15;
  const int wr = w >> 1, wc = w & 1;
  const int v = (int)(blockIdx.x % (unsigned)a.W), grp = (int)(blockIdx.x / (unsigned)a.W);
  const int p0 = a.item_p0[v], q0 = T * a.item_tile[v];
  const int b0 = PB * grp;
  const int npb = a.nb - b0 < PB ? a.nb - b0 : PB;         // the group's permutations: >= 1 by the grid
  const int n = a.n;
  const size_t ystride = (size_t)a.qa * (size_t)n;
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
    const int j = q0 + (int)threadIdx.x;
    const bool tv = j < a.qa;
    ts_syy[threadIdx.x] = tv ? a.syy[j] : 0.0;
    ts_m[threadIdx.x] = tv ? a.mt[j] : 0;
    ts_lo[threadIdx.x] = tv ? a.lo[j] : 0;
    ts_hi[threadIdx.x] = tv ? a.hi[j] : 0;
    ts_orig[threadIdx.x] = tv ? a.orig[j] : 0;
  }
  double2 vx[SH::NV], vy[PB][SH::NV];
  aq_ms_load<T, A16>(a.Xs, n, a.p1, p0, 0, vx);
#pragma unroll
  for (int pb = 0; pb < PB; pb++)
    if (pb < npb) aq_ms_load<T, A16>(a.Yo + (size_t)(b0 + pb) * ystride, n, a.qa, q0, 0, vy[pb]);
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
        if (pb < npb) aq_ms_load<T, A16>(a.Yo + (size_t)(b0 + pb) * ystride, n, a.qa, q0, i0 + AQ_MSCREEN_NC, vy[pb]);
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

  // ---- epilogue: the largest in-window r^2 per permutation and trait ----
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
#pragma unroll
      for (int i = 0; i < NI; i++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const int tl = wr * SH::WT + 16 * i + g + 4 * reg;
          const double syy = ts_syy[tl];
          const int m = ts_m[tl], lo = ts_lo[tl], hi = ts_hi[tl];
          const double md = (double)m;
          const bool t_ok = m - 2 - a.n_cov >= 1 && syy > 0.0;
          double br2 = -1.0;
#pragma unroll
          for (int jj = 0; jj < NI; jj++) {
            const int s = p0 + wc * SH::WT + 16 * jj + l;
            if (t_ok && s >= lo && s < hi) {
              const double sxy = axy[pb][i][jj][reg];
              const double sx = MASKED ? ax[pb][i % NS][jj % NS][reg] : csx[jj];
              const double sxx = MASKED ? axx[pb][i % NS][jj % NS][reg] : csxx[jj];
              const double vx = sxx - sx * sx / md;
              if (vx > 1e-10 * sxx) {
                const double r = sxy / sqrt(vx * syy);
                const double r2 = r * r;
                if (r2 > br2) br2 = r2;
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
    }
  __syncthreads();
  for (int idx = threadIdx.x; idx < PB * T; idx += 256) {   // the two waves of a tile row, then the items of the trait tile
    const int pb = idx / T, tl = idx % T;
    if (pb < npb && q0 + tl < a.qa) {
      const double m0 = cmax[0][pb][tl], m1 = cmax[1][pb][tl];
      const double mx = m1 > m0 ? m1 : m0;
      if (mx >= 0.0)
        atomicMax(a.key + (size_t)(b0 + pb) * (size_t)a.q + (size_t)ts_orig[tl], (unsigned long long)__double_as_longlong(mx) + 1ull);
    }
  }
}

static __global__ __launch_bounds__(256) void aq_k_cis_reduce(const unsigned long long *__restrict__ key, long long count,
                                                             double *__restrict__ max_r2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const unsigned long long k = key[i];
  max_r2[i] = k ? __longlong_as_double((long long)(k - 1ull)) : -1.0;
}
