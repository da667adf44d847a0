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
// aq_k_cc_tile<KC, A16>, KC in {1, 2, 4}, grid W, 256 threads, over the work items of aq_cis_plan.h: the loop of aq_screen_tile.h
// with 1 + KC trait-side panels, the residual traits of Yo and the KC basis panels of Qo, and as many accumulator sets fed
// from the same operand read of X: acc_0 += Y~ X and acc_j += Q_j X.  tile_k[k] is the largest k_eff of trait tile k: a
// workgroup neither loads, stages nor multiplies a basis panel j >= tile_k (all zeros), which is uniform over the workgroup
// and leaves its accumulators at 0.0, the value the products of zeros would have given.  32 accumulator registers per set,
// 160 at KC = 4; LDS (2 + KC) 64 18 8 bytes plus the per-trait arrays (aq_ciscond_lds_bytes).
// The epilogue is aq_cis_scan_epilogue of aq_cis_kernels.h with `lost` = a_1^2 + ... + a_KC^2 handed to aq_ms_pair, its
// roundings spelled out in the kernel; aq_k_cis_best then reduces over a tile's items.
#pragma once
#include "aq_ciscond_plan.h"
#include "aq_cis_kernels.h"       // aq_cis_args, AqCisWin, aq_cis_scan_epilogue; aq_screen_tile.h

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
  __shared__ __attribute__((aligned(16))) double PX[SH::PAN];
  __shared__ __attribute__((aligned(16))) double PT[(1 + KC) * SH::PAN];   // the residual traits, then the KC basis panels
  __shared__ double cand_r[2][T];
  __shared__ int cand_s[2][T];
  __shared__ double ts_syy[T], ts_cut[T];                  // S~yy_t and the cutoff; not testable for a trait >= qa
  __shared__ int ts_ok[T];
  __shared__ AqCisWin win;
  static_assert(sizeof(double) * ((2 + KC) * SH::PAN) + 2 * T * 12 + T * 32 == aq_ciscond_lds_bytes(KC), "plan and kernel");
  static_assert(sizeof(AqCisWin) == T * 12 && aq_ciscond_lds_bytes(KC) <= 65536, "64 KB of static LDS");
  const aq_cis_args &a = ca.c;
  const AqMsLane ln;
  const int p0 = a.item_p0[blockIdx.x], kt = a.item_tile[blockIdx.x], q0 = T * kt;
  const int nq = ca.tile_k[kt];                            // basis panels of this trait tile that hold anything: <= KC
  const int n = a.n;
  const size_t qpanel = (size_t)a.qa * (size_t)n;
  if ((int)threadIdx.x < T) {
    aq_ms_trait_fill(ts_syy, a.syy, q0, a.qa);
    aq_ms_trait_fill(ts_cut, a.cut, q0, a.qa);
    win.fill(a, q0);
    const int j = q0 + (int)threadIdx.x;
    ts_ok[threadIdx.x] = j < a.qa && n - 2 - a.n_cov - ca.keff[j] >= 1 && a.syy[j] > 1e-10 * ca.syy0[j];
  }
  aq_ms_acc<T, 1 + KC> acc;                                // [0]: x_s' y~_t; [j]: a_j = q_tj' x_s
  aq_ms_acc_m<T, false, 1 + KC> unused_x, unused_xx;
  // GUARD = 1: the residual traits (panel 0) are always live, the basis panels k >= 1 are tested against 1 + nq
  aq_ms_tile_loop<T, false, A16, 1 + KC, 1, AQ_MS_STEP_PLAIN>(a.Xs, n, a.p1, p0, a.qa, q0, 1 + nq,
                                               [&](int k) { return k == 0 ? a.Yo : ca.Qo + (size_t)(k - 1) * qpanel; }, PX, PT, acc,
                                               unused_x, unused_xx);
  const double nd = (double)n;
  double csx[SH::NI], csxx[SH::NI];
  aq_ms_col_sums<SH::NI, true>(a.sx, a.sxx, p0 + ln.wc * SH::WT + ln.l, a.p1, csx, csxx);
  const auto trait = [&](int tl) { return AqCisTrait{ts_ok[tl] != 0, ts_syy[tl], nd}; };
  aq_cis_scan_epilogue(a, p0, q0, ts_cut, win, cand_r, cand_s, trait, [&](int i, int jj, int reg, const AqCisTrait &tr, double *r) {
    // The variance of x_s that the conditioning takes, a_1^2 + ... + a_KC^2.  Which product of a sum of products the compiler
    // folds into a fused multiply-add is its choice and moves the last bit of r, so the choice is spelled out here: a_2^2 is
    // rounded, a_1^2 is folded onto it, then a_3^2 and a_4^2 in this order (what the first build of this kernel computed).
    // Not pinned: at KC = 1 `lost` is one product, and whether Vx0 - a_1^2 inside aq_ms_pair becomes one fused operation is
    // still the compiler's choice (HIP's default contraction); the other kernels pass 0.0 and have nothing to contract.
    constexpr int C2 = KC > 1 ? 2 : 1;
    const double a1 = acc[1][i][jj][reg], a2 = acc[C2][i][jj][reg];
    double lost = KC > 1 ? __builtin_fma(a1, a1, a2 * a2) : a1 * a1;
#pragma unroll
    for (int c = 3; c <= KC; c++) lost = __builtin_fma(acc[c][i][jj][reg], acc[c][i][jj][reg], lost);
    return aq_ms_pair(acc[0][i][jj][reg], csx[jj], csxx[jj], tr.m, tr.syy, lost, r);
  });
}
