// aq_ciscond_kernels.h -- the conditional cis scan of a finished prepare handle: every in-window pair
// (predictor s, trait t) tested after the trait's own conditioning variants have been regressed out of both, which asks whether
// a second signal sits in the window or only LD proxies of the first.  Included by aq_prep_cis_cond.hip alone; the launch plan
// is aq_ciscond_plan.h, the order of the traits and the work items those of aq_cis_plan.h.  Every kernel is a plain grid: no
// workgroup waits for another one, nothing spins, and no floating-point atomic is used (the integer atomics are counters), so
// two calls give the same set of rows and the same bits everywhere else.
//
// The statistic (include/atlasqtl_hip.h, aq_prep_cis_cond).  Complete Y only.  Xs and Yc are the prepared matrices of the
// handle, centred and, with covariates, residualised; n_cov as in aq_prep_marginal.  Trait t has a conditioning list C_t of
// 0 <= k_t <= 4 distinct predictor indices in [0, p1), in the order given, independent of the trait's window.
//   Basis.  Go through C_t in order.  v = Xs[:, c].  Project out the basis vectors accepted so far, twice: in each of two
//   passes, for every accepted q in the order of acceptance, v <- v - q (q'v) (Gram-Schmidt with one re-orthogonalisation).
//   If |v|^2 <= 1e-10 |Xs[:, c]|^2 the column is dropped: a conditioning variant collinear with the earlier ones.  Otherwise
//   q = v / |v| is accepted.  k_eff[t] is the number accepted.
//   Residual trait.  y~_t = y_t - sum_j q_tj (q_tj' y_t), S~yy_t = sum y~^2.  With k_eff = 0, y~_t is the copy of y_t.
//   Per pair with s_lo[t] <= s < s_hi[t]:  a_j = q_tj' x_s;  Vx = (Sxx - Sx^2 / n) - (a_1^2 + ... + a_k^2), the parenthesis
//   evaluated first, exactly as the plain scan does;  r = (x_s' y~_t) / sqrt(Vx S~yy_t);  df_t = n - 2 - n_cov - k_eff[t].
//   Undefined pairs.  A pair is undefined when Vx <= 1e-10 Sxx, when S~yy_t <= 1e-10 Syy_t, or when df_t < 1.  Its r is NaN;
//   it is counted and never selected.  The first condition removes each conditioning variant from its own trait's tests, and
//   anything collinear with the list.
//
// aq_k_cc_basis, grid q_active, 256 threads: workgroup j owns the ordered trait j.  Thread i owns the samples i, i + 256, ... of
// every vector of the trait, so the only exchange between threads is the length-n sums, each through aq_block_sum in its fixed
// order.  It gathers the trait's <= 4 columns of Xs (each contiguous in [p1][n]), builds Q and y~ as defined above in place in
// Qo[j'][ordered trait][n] (zeros for j' >= k_eff, up to KC) and Yo[ordered trait][n], and writes S~yy (ordered) and k_eff
// (under the trait's own index).  Qo is KC panels of the shape of Yo, [q_active][n] each, so aq_ms_load<64, A16> reads each of
// the 1 + KC trait-side panels unchanged.  A trait with k_t = 0, or with k_eff = 0, is a plain copy of y: no arithmetic on y,
// and S~yy_t is the Syy_t of aq_k_ms_traitstats that the plain scan uses, so that its r is the plain scan's to the bit.
//
// aq_k_cc_tile<KC, A16>, KC in {1, 2, 4}, grid W, 256 threads, over the work items of aq_cis_plan.h.  The loop is that of
// aq_k_cis_tile<false, A16> with 1 + KC trait-side LDS panels (rows of AQ_MSCREEN_STR doubles: the bank argument of
// aq_mscreen_kernels.h holds for each) and 1 + KC accumulator sets fed from the same x[jj] registers: acc_y += Y~ X and
// acc_j += Q_j X, 1 + KC streams of f64 matrix instructions from one operand read of X.  tile_k[k] is the largest k_eff of
// trait tile k: a workgroup neither loads, stages nor multiplies a basis panel j >= tile_k (all zeros), which is uniform over
// the workgroup and leaves its accumulators at 0.0, the value the products of zeros would have given.  32 accumulator
// registers per set, 160 at KC = 4; LDS (2 + KC) 64 18 8 bytes plus the per-trait arrays (aq_ciscond_lds_bytes).
// The epilogue is that of aq_k_cis_tile with Vx as above, the squares added in the order j = 1 ... KC: the selected-pair table
// through one 64-bit counter, per-trait undefined counts, the item's best predictor per trait with ties to the lowest index;
// aq_k_cis_best then reduces over a tile's items.
#pragma once
#include "aq_ciscond_plan.h"
#include "aq_cis_kernels.h"       // aq_cis_args; aq_mscreen_kernels.h: aq_ms_d4, AqMsShape, aq_ms_load, aq_ms_store; aq_block_sum

struct aq_cc_args {
  aq_cis_args c;                  // Yo: the residual traits; syy: S~yy_t; mt is not read (complete Y: m_t = n)
  const double *Qo;               // [KC][qa][n]
  const double *syy0;             // per ordered trait: Syy_t of the trait itself
  const int32_t *keff;            // per ordered trait
  const int32_t *tile_k;          // per trait tile: the largest k_eff of its traits
};

// ck[j], cidx[4 j ...]: the list of ordered trait j.  syy0: Syy_t per ordered trait.  keff_o: ordered; keff_t: by the trait's index.
static __global__ __launch_bounds__(256) void aq_k_cc_basis(const double *__restrict__ Xs, const double *__restrict__ Yc,
                                                           const int32_t *__restrict__ order, const int32_t *__restrict__ ck,
                                                           const int32_t *__restrict__ cidx, const double *__restrict__ syy0, int n, int qa,
                                                           int kc, double *Qo, double *__restrict__ Yo, double *__restrict__ syyt,
                                                           int32_t *__restrict__ keff_o, int32_t *__restrict__ keff_t) {
  __shared__ double sh[256];
  const int j = blockIdx.x, t = order[j], k = ck[j];
  const size_t panel = (size_t)qa * (size_t)n;
  const double *y = Yc + (size_t)t * (size_t)n;
  double *yo = Yo + (size_t)j * (size_t)n;
  int kacc = 0;
  for (int c = 0; c < k; c++) {
    const double *col = Xs + (size_t)cidx[AQ_CISCOND_KMAX * j + c] * (size_t)n;
    double *v = Qo + (size_t)kacc * panel + (size_t)j * (size_t)n;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
      const double x = col[i];
      v[i] = x;
      s += x * x;
    }
    const double norm0 = aq_block_sum(s, sh);
    for (int pass = 0; pass < 2; pass++)
      for (int m = 0; m < kacc; m++) {
        const double *qm = Qo + (size_t)m * panel + (size_t)j * (size_t)n;
        double d = 0.0;
        for (int i = threadIdx.x; i < n; i += 256) d += qm[i] * v[i];
        d = aq_block_sum(d, sh);
        for (int i = threadIdx.x; i < n; i += 256) v[i] -= qm[i] * d;
      }
    s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += v[i] * v[i];
    const double nv = aq_block_sum(s, sh);
    if (nv > 1e-10 * norm0) {                      // the same value in every thread: uniform
      const double len = sqrt(nv);
      for (int i = threadIdx.x; i < n; i += 256) v[i] = v[i] / len;
      kacc++;
    }
  }
  for (int m = kacc; m < kc; m++) {                // also what a dropped column left in slot kacc
    double *z = Qo + (size_t)m * panel + (size_t)j * (size_t)n;
    for (int i = threadIdx.x; i < n; i += 256) z[i] = 0.0;
  }
  double st = syy0[j];
  if (kacc == 0) {
    for (int i = threadIdx.x; i < n; i += 256) yo[i] = y[i];
  } else {
    double d[AQ_CISCOND_KMAX];
#pragma unroll
    for (int m = 0; m < AQ_CISCOND_KMAX; m++) {
      d[m] = 0.0;
      if (m < kacc) {
        const double *qm = Qo + (size_t)m * panel + (size_t)j * (size_t)n;
        double a = 0.0;
        for (int i = threadIdx.x; i < n; i += 256) a += qm[i] * y[i];
        d[m] = aq_block_sum(a, sh);
      }
    }
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
      double r = y[i];
#pragma unroll
      for (int m = 0; m < AQ_CISCOND_KMAX; m++)
        if (m < kacc) r -= Qo[(size_t)m * panel + (size_t)j * (size_t)n + i] * d[m];
      yo[i] = r;
      s += r * r;
    }
    st = aq_block_sum(s, sh);
  }
  if (threadIdx.x == 0) {
    syyt[j] = st;
    keff_o[j] = kacc;
    keff_t[t] = kacc;
  }
}

// KC = 4: 160 accumulator registers and five staged panels in flight; the register report of the build is in DESIGN.md section 9
template <int KC, bool A16>
__global__ __launch_bounds__(256, 2) void aq_k_cc_tile(const aq_cc_args ca) {
  static_assert(aq_ciscond_instance(KC), "an instance of the plan");
  constexpr int T = AQ_CIS_TILE;
  typedef AqMsShape<T> SH;
  constexpr int NI = SH::NI;
  constexpr int PAN = T * SH::STR;                         // doubles of a panel
  __shared__ __attribute__((aligned(16))) double PX[PAN];
  __shared__ __attribute__((aligned(16))) double PT[(1 + KC) * PAN];   // the residual traits, then the KC basis panels
  __shared__ double cand_r[2][T];
  __shared__ int cand_s[2][T];
  __shared__ double ts_syy[T], ts_cut[T];                  // S~yy_t and the cutoff; not testable and an empty window for a trait >= qa
  __shared__ int ts_ok[T], ts_lo[T], ts_hi[T], ts_orig[T];
  static_assert(sizeof(double) * ((2 + KC) * PAN) + 2 * T * 12 + T * 32 == aq_ciscond_lds_bytes(KC), "plan and kernel");
  static_assert(aq_ciscond_lds_bytes(KC) <= 65536, "64 KB of static LDS");
  const aq_cis_args &a = ca.c;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, l = lane & 15;
  const int wr = w >> 1, wc = w & 1;
  const int p0 = a.item_p0[blockIdx.x], kt = a.item_tile[blockIdx.x], q0 = T * kt;
  const int nq = ca.tile_k[kt];                            // basis panels of this trait tile that hold anything: <= KC
  const int n = a.n;
  const size_t qpanel = (size_t)a.qa * (size_t)n;
  aq_ms_d4 axy[NI][NI], aq[KC][NI][NI];
#pragma unroll
  for (int i = 0; i < NI; i++)
#pragma unroll
    for (int jj = 0; jj < NI; jj++) {
      axy[i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < KC; c++) aq[c][i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
    }
  const int toff = (wr * SH::WT + l) * SH::STR + g;        // the lane's first operand within a trait-side panel
  const double *px = PX + (wc * SH::WT + l) * SH::STR + g;
  if ((int)threadIdx.x < T) {                      // read after the loop's barriers
    const int j = q0 + (int)threadIdx.x;
    const bool tv = j < a.qa;
    const double st = tv ? a.syy[j] : 0.0;
    ts_syy[threadIdx.x] = st;
    ts_cut[threadIdx.x] = tv ? a.cut[j] : 0.0;
    ts_ok[threadIdx.x] = tv && n - 2 - a.n_cov - ca.keff[j] >= 1 && st > 1e-10 * ca.syy0[j];
    ts_lo[threadIdx.x] = tv ? a.lo[j] : 0;
    ts_hi[threadIdx.x] = tv ? a.hi[j] : 0;
    ts_orig[threadIdx.x] = tv ? a.orig[j] : 0;
  }
  double2 vx[SH::NV], vt[1 + KC][SH::NV];
  aq_ms_load<T, A16>(a.Xs, n, a.p1, p0, 0, vx);
  aq_ms_load<T, A16>(a.Yo, n, a.qa, q0, 0, vt[0]);
#pragma unroll
  for (int c = 0; c < KC; c++)
    if (c < nq) aq_ms_load<T, A16>(ca.Qo + (size_t)c * qpanel, n, a.qa, q0, 0, vt[1 + c]);
  for (int i0 = 0; i0 < n; i0 += AQ_MSCREEN_NC) {
    __syncthreads();                             // the panels of the previous chunk have been read
    aq_ms_store<T>(vx, PX);
    aq_ms_store<T>(vt[0], PT);
#pragma unroll
    for (int c = 0; c < KC; c++)
      if (c < nq) aq_ms_store<T>(vt[1 + c], PT + (1 + c) * PAN);
    __syncthreads();
    if (i0 + AQ_MSCREEN_NC < n) {
      aq_ms_load<T, A16>(a.Xs, n, a.p1, p0, i0 + AQ_MSCREEN_NC, vx);
      aq_ms_load<T, A16>(a.Yo, n, a.qa, q0, i0 + AQ_MSCREEN_NC, vt[0]);
#pragma unroll
      for (int c = 0; c < KC; c++)
        if (c < nq) aq_ms_load<T, A16>(ca.Qo + (size_t)c * qpanel, n, a.qa, q0, i0 + AQ_MSCREEN_NC, vt[1 + c]);
    }
#pragma unroll
    for (int kk = 0; kk < AQ_MSCREEN_NC; kk += 4) {
      double x[NI], y[NI];
#pragma unroll
      for (int i = 0; i < NI; i++) {
        x[i] = px[16 * i * SH::STR + kk];
        y[i] = PT[toff + 16 * i * SH::STR + kk];
      }
#pragma unroll
      for (int i = 0; i < NI; i++)
#pragma unroll
        for (int jj = 0; jj < NI; jj++) axy[i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[i], x[jj], axy[i][jj], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < KC; c++)
        if (c < nq) {
          double qv[NI];
#pragma unroll
          for (int i = 0; i < NI; i++) qv[i] = PT[(1 + c) * PAN + toff + 16 * i * SH::STR + kk];
#pragma unroll
          for (int i = 0; i < NI; i++)
#pragma unroll
            for (int jj = 0; jj < NI; jj++) aq[c][i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[i], x[jj], aq[c][i][jj], 0, 0, 0);
        }
    }
  }

  // ---- epilogue: r of the wave's 32 x 32 pairs, four traits (g + 4 reg) x one predictor (l) per accumulator and lane ----
  const double nd = (double)n;
  double csx[NI], csxx[NI];                        // Sx and Sxx of the lane's predictors
#pragma unroll
  for (int jj = 0; jj < NI; jj++) {
    const int s = p0 + wc * SH::WT + 16 * jj + l;
    csx[jj] = s < a.p1 ? a.sx[s] : 0.0;
    csxx[jj] = s < a.p1 ? a.sxx[s] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < NI; i++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int tl = wr * SH::WT + 16 * i + g + 4 * reg;
      const double syy = ts_syy[tl], cut = ts_cut[tl];
      const int lo = ts_lo[tl], hi = ts_hi[tl], t = ts_orig[tl];
      const bool t_ok = ts_ok[tl] != 0;
      double br2 = -1.0, br = __builtin_nan("");
      int bs = 0x7fffffff;
      unsigned int undef = 0;
#pragma unroll
      for (int jj = 0; jj < NI; jj++) {
        const int s = p0 + wc * SH::WT + 16 * jj + l;
        if (s >= lo && s < hi) {                   // hi <= p1, and lo = hi = 0 for a trait >= qa: the pair exists
          double r = __builtin_nan("");
          bool ok = false;
          if (t_ok) {
            const double sxy = axy[i][jj][reg];
            double lost = 0.0;                     // the variance of x_s that the conditioning takes
#pragma unroll
            for (int c = 0; c < KC; c++) lost += aq[c][i][jj][reg] * aq[c][i][jj][reg];
            const double sxx = csxx[jj];
            const double vx0 = sxx - csx[jj] * csx[jj] / nd;
            const double vx = vx0 - lost;
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
