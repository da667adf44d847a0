// aq_cisint_kernels.h -- the interaction cis scan of a finished prepare handle: for every in-window pair
// (predictor s, trait t) the partial correlation of the interaction term g o e with the trait given the intercept, the
// covariates, e and g itself, which asks whether the effect of the variant depends on a sample-level variable (tensorQTL's
// map_cis(interaction_df=)).  Included by aq_prep_cis_int.hip alone; the launch plan is aq_cisint_plan.h, the order of the
// traits and the work items those of aq_cis_plan.h.  Every kernel is a plain grid: no workgroup waits for another one, nothing
// spins, and no floating-point atomic is used (the integer atomics are counters), so two calls give the same set of rows and
// the same bits everywhere else.
//
// The statistic (include/atlasqtl_hip.h, aq_prep_cis_int).  Complete Y only.  Xs [p1][n] and Yc [q][n] are the handle's
// prepared matrices.  B is nb orthonormal n-vectors spanning [1, Z, e], Z the covariates the handle was prepared with,
// nb = n_cov + 2; m is the per-sample multiplier, e centred.
//   Per trait t:      y' = y_t - sum_k b_k (b_k'y_t), in the order of B;  S'yy_t = sum y'^2;  S0yy_t = the Syy_t of
//                     aq_k_ms_traitstats.
//   Per predictor s,  g = Xs[:, s], w = g o m, every product rounded once:  a_k = b_k'g, c_k = b_k'w, Sxx = g'g, Sww = w'w,
//                     Vg = Sxx - sum a_k^2,  Cgw = g'w - sum a_k c_k,  Vw = Sww - sum c_k^2 - Cgw^2 / Vg.
//   Per in-window pair:  Sgy = g'y', Swy = w'y' (the two matrix-instruction streams);  num = Swy - (Cgw / Vg) Sgy;
//                     S'' = S'yy - Sgy^2 / Vg;  r = num / sqrt(Vw S'');  df = n - nb - 2.
//   Undefined pairs.  Vg <= 1e-10 Sxx, Vw <= 1e-10 Sww, S'' <= 1e-10 S0yy_t or df < 1.  r is NaN; the pair is counted and
//                     never selected.
//
// aq_k_ci_traits, grid q_active, 256 threads: workgroup j owns the ordered trait j.  Thread i owns the samples i, i + 256, ...;
// the nb dot products b_k'y_t, each through aq_block_sum in its fixed order, are kept in LDS; then y' is written into
// Yo[ordered trait][n], the products taken off in the order of B, and S'yy through aq_block_sum.
//
// aq_k_ci_predstats, grid p1, 256 threads: the workgroup of predictor s forms a_k, c_k (k in the order of B), Sxx, Sww and
// g'w, each length-n sum through aq_block_sum, w_i = g_i m_i rounded once wherever it is used; then, the same in every
// thread, Vg, Cgw / Vg and Vw in the order of roundings written out in the kernel, whether the predictor is defined, and
// int_tol = Vw / Sww (NaN for a predictor that is not).
//
// aq_k_ci_tile<A16>, grid W, 256 threads, over the work items of aq_cis_plan.h: aq_ms_tile_loop_x2 of aq_screen_tile.h, one
// staged panel of X and one trait-side panel (Yo), two accumulator sets acc0 += Y' x and acc1 += Y' (x m_i), the multiplier
// read from the zero-padded copy of mult.  64 accumulator registers; LDS two panels plus the per-trait arrays
// (aq_cisint_lds_bytes).  The epilogue is aq_cis_scan_epilogue of aq_cis_kernels.h with the pair formula above as its `stat`,
// the roundings spelled out in the kernel; aq_k_cis_best then reduces over a tile's items.
#pragma once
#include "aq_cisint_plan.h"
#include "aq_cis_kernels.h"       // aq_cis_args, AqCisWin, AqCisTrait, aq_cis_scan_epilogue; aq_screen_tile.h

struct aq_ci_args {
  aq_cis_args c;                  // Yo: the residual traits; syy: S'yy_t; mt, sx and sxx are not read
  const double *mpad;             // the multiplier, zero-padded to aq_cisint_mult_pad(n) doubles
  const double *syy0;             // per ordered trait: S0yy_t, the trait's own
  const double *vg, *cgv, *vw;    // per predictor: Vg, Cgw / Vg, Vw
  const int32_t *pok;             // per predictor: Vg > 1e-10 Sxx and Vw > 1e-10 Sww
  int nb;                         // basis vectors: df = n - nb - 2
};

// B: [nb][n].  syyt: S'yy per ordered trait.
static __global__ __launch_bounds__(256) void aq_k_ci_traits(const double *__restrict__ Yc, const int32_t *__restrict__ order,
                                                            const double *__restrict__ B, int n, int nb, double *__restrict__ Yo,
                                                            double *__restrict__ syyt) {
  __shared__ double sh[256];
  __shared__ double d[AQ_CISINT_NB_MAX];
  const int j = blockIdx.x;
  const double *y = Yc + (size_t)order[j] * (size_t)n;
  double *yo = Yo + (size_t)j * (size_t)n;
  for (int k = 0; k < nb; k++) {
    const double *bk = B + (size_t)k * (size_t)n;
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += bk[i] * y[i];
    a = aq_block_sum(a, sh);
    if (threadIdx.x == 0) d[k] = a;
  }
  __syncthreads();
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    double r = y[i];
    for (int k = 0; k < nb; k++) r -= B[(size_t)k * (size_t)n + i] * d[k];
    yo[i] = r;
    s += r * r;
  }
  s = aq_block_sum(s, sh);
  if (threadIdx.x == 0) syyt[j] = s;
}

static __global__ __launch_bounds__(256) void aq_k_ci_predstats(const double *__restrict__ Xs, const double *__restrict__ B,
                                                               const double *__restrict__ mult, int n, int nb, double *__restrict__ vg,
                                                               double *__restrict__ cgv, double *__restrict__ vw, int32_t *__restrict__ pok,
                                                               double *__restrict__ int_tol) {
  __shared__ double sh[256];
  const double *g = Xs + (size_t)blockIdx.x * (size_t)n;
  double sxx = 0.0, sww = 0.0, sgw = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double x = g[i];
    const double w = x * mult[i];                // rounded once: the tile kernel's second operand
    sxx += x * x;
    sww += w * w;
    sgw += x * w;
  }
  sxx = aq_block_sum(sxx, sh);
  sww = aq_block_sum(sww, sh);
  sgw = aq_block_sum(sgw, sh);
  // The sums over the basis, the same in every thread.  Which product of a sum of products the compiler folds into a fused
  // multiply-add is its choice and moves the last bit, so the choice is spelled out: every a_k^2, a_k c_k and c_k^2 is folded
  // onto the running sum, k ascending.
  double sa2 = 0.0, sac = 0.0, sc2 = 0.0;
  for (int k = 0; k < nb; k++) {
    const double *bk = B + (size_t)k * (size_t)n;
    double a = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
      const double x = g[i];
      const double w = x * mult[i];
      a += bk[i] * x;
      c += bk[i] * w;
    }
    a = aq_block_sum(a, sh);
    c = aq_block_sum(c, sh);
    sa2 = __builtin_fma(a, a, sa2);
    sac = __builtin_fma(a, c, sac);
    sc2 = __builtin_fma(c, c, sc2);
  }
  if (threadIdx.x == 0) {
    // Vg = Sxx - sum a_k^2 and Cgw = g'w - sum a_k c_k: one subtraction each.  Cgw / Vg: one division.  Vw = (Sww - sum c_k^2)
    // - Cgw (Cgw / Vg): the parenthesis first, then the product folded onto it.
    const double v = sxx - sa2;
    const double cgw = sgw - sac;
    const bool gok = v > 1e-10 * sxx;
    const double ratio = gok ? cgw / v : 0.0;
    const double w0 = sww - sc2;
    const double vwv = __builtin_fma(-cgw, ratio, w0);
    const bool ok = gok && vwv > 1e-10 * sww;
    vg[blockIdx.x] = v;
    cgv[blockIdx.x] = ratio;
    vw[blockIdx.x] = vwv;
    pok[blockIdx.x] = ok ? 1 : 0;
    int_tol[blockIdx.x] = ok ? vwv / sww : __builtin_nan("");
  }
}

// two accumulator sets of 32 registers, two staged panels in flight; the register report of the build is in DESIGN.md section 9
template <bool A16>
__global__ __launch_bounds__(256, 2) void aq_k_ci_tile(const aq_ci_args ca) {
  constexpr int T = AQ_CIS_TILE;
  typedef AqMsShape<T> SH;
  __shared__ __attribute__((aligned(16))) double PX[SH::PAN];
  __shared__ __attribute__((aligned(16))) double PT[SH::PAN];   // the residual traits
  __shared__ double cand_r[2][T];
  __shared__ int cand_s[2][T];
  __shared__ double ts_syy[T], ts_cut[T], ts_floor[T];     // S'yy_t, the cutoff, 1e-10 S0yy_t; not testable for a trait >= qa
  __shared__ int ts_ok[T];
  __shared__ AqCisWin win;
  static_assert(sizeof(double) * (2 * SH::PAN) + 2 * T * 12 + T * 40 == aq_cisint_lds_bytes(), "plan and kernel");
  static_assert(sizeof(AqCisWin) == T * 12 && aq_cisint_lds_bytes() <= 65536, "64 KB of static LDS");
  const aq_cis_args &a = ca.c;
  const AqMsLane ln;
  const int p0 = a.item_p0[blockIdx.x], q0 = T * a.item_tile[blockIdx.x];
  const int n = a.n;
  if ((int)threadIdx.x < T) {
    aq_ms_trait_fill(ts_syy, a.syy, q0, a.qa);
    aq_ms_trait_fill(ts_cut, a.cut, q0, a.qa);
    win.fill(a, q0);
    const int j = q0 + (int)threadIdx.x;
    ts_floor[threadIdx.x] = j < a.qa ? 1e-10 * ca.syy0[j] : 0.0;
    ts_ok[threadIdx.x] = j < a.qa && n - ca.nb - 2 >= 1;
  }
  aq_ms_acc<T, 1> acc0, acc1;                              // Sgy = g'y' and Swy = w'y'
  aq_ms_tile_loop_x2<T, A16>(a.Xs, n, a.p1, p0, a.Yo, a.qa, q0, ca.mpad, PX, PT, acc0, acc1);
  double pvg[SH::NI], pcgv[SH::NI], pvw[SH::NI];
  bool pok[SH::NI];
#pragma unroll
  for (int jj = 0; jj < SH::NI; jj++) {
    const int s = p0 + ln.wc * SH::WT + ln.l + 16 * jj;
    const bool in = s < a.p1;
    pvg[jj] = in ? ca.vg[s] : 1.0;
    pcgv[jj] = in ? ca.cgv[s] : 0.0;
    pvw[jj] = in ? ca.vw[s] : 1.0;
    pok[jj] = in && ca.pok[s] != 0;
  }
  // AqCisTrait: syy carries S'yy_t and m, which the plain scan fills with m_t, the floor of S'', 1e-10 S0yy_t
  const auto trait = [&](int tl) { return AqCisTrait{ts_ok[tl] != 0, ts_syy[tl], ts_floor[tl]}; };
  aq_cis_scan_epilogue(a, p0, q0, ts_cut, win, cand_r, cand_s, trait, [&](int i, int jj, int reg, const AqCisTrait &tr, double *r) {
    // The pair statistic.  num and S'' each hold a cancellation, and which product the compiler folds into a fused
    // multiply-add moves the last bits of r, so the roundings are spelled out:
    //   num = Swy - (Cgw / Vg) Sgy       the product folded onto Swy: one rounding;
    //   S'' = S'yy - Sgy (Sgy / Vg)      the quotient rounded, its product with Sgy folded onto S'yy: two roundings;
    //   r   = num / sqrt(Vw S'')         a product, a square root, a division.
    // Vw and Cgw / Vg come from aq_k_ci_predstats, where their roundings are written out.
    const double sgy = acc0[0][i][jj][reg], swy = acc1[0][i][jj][reg];
    const double num = __builtin_fma(-pcgv[jj], sgy, swy);
    const double s2 = __builtin_fma(-sgy, sgy / pvg[jj], tr.syy);
    const bool ok = pok[jj] && s2 > tr.m;
    if (ok) *r = num / sqrt(pvw[jj] * s2);
    return ok;
  });
}
