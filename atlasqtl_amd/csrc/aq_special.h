// aq_special.h -- fp64 special functions used on the VB path, written once for
// device (hipcc) and host (g++, for the CPU unit tests in tests/test_special.py).
//
// Reference call sites these replace (the reference gets them from base R / GSL,
// whose sources are not part of the reference repository):
//   aq_log_ndtr      pnorm(x, log.p = TRUE)                R/atlasqtl_global_local_core.R:62-63,294-295, R/update_vb.R:223-224
//   aq_digamma       digamma()                             R/update_vb.R:120,159
//   aq_expint_e1     gsl::expint_E1 (x <= 1 branch)        R/utils.R:387
//   aq_lentz_*       the modified-Lentz loop for x > 1     R/utils.R:392-419
//   aq_gamma_inc_upper  gsl::gamma_inc(a, x), a in (0, 2)  R/update_vb.R:74
//   aq_sigmoid_neg   exp(-logOnePlusExp(x))                src/coreLoop.cpp:28-33,75-77
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AQ_HD __host__ __device__ __forceinline__
#else
#define AQ_HD static inline
#endif

#define AQ_LOG_SQRT_2PI 0.91893853320467274178032973640562
#define AQ_INV_SQRT2 0.70710678118654752440084436210485
#define AQ_EULER_GAMMA 0.57721566490153286060651209008240
#define AQ_SQRT_2_OVER_PI 0.79788456080286535587989211986876
#define AQ_INV_SQRT_2PI 0.39894228040143267793994605993438
#include "aq_erfcx_coef.h"
#include "aq_probit_tab.h"

// log Phi(x).  x > 0: log1p(-erfc(x/sqrt2)/2); -37 < x <= 0: log(erfc(-x/sqrt2)/2)
// (erfc keeps full relative accuracy in its tail until it underflows near 26.5);
// x <= -37: asymptotic Mills-ratio series.
AQ_HD double aq_log_ndtr(double x) {
  if (x > 0.0) return log1p(-0.5 * erfc(x * AQ_INV_SQRT2));
  if (x > -37.0) return log(0.5 * erfc(-x * AQ_INV_SQRT2));
  double ix2 = 1.0 / (x * x);
  // 1 - 1/x^2 + 3/x^4 - 15/x^6 + 105/x^8 - 945/x^10
  double ser = 1.0 + ix2 * (-1.0 + ix2 * (3.0 + ix2 * (-15.0 + ix2 * (105.0 - 945.0 * ix2))));
  return -0.5 * x * x - log(-x) - AQ_LOG_SQRT_2PI + log(ser);
}

// Phi^-1(u) for 0 < u <= 1/2 (the lower half: the caller mirrors the upper one, so that u and 1 - u give exact negatives);
// u = 1/2 gives exactly 0, u = 0 gives -inf, anything else outside the range NaN.  qnorm(u) of R.
// No table: the three-term rational start of Abramowitz & Stegun 26.2.23 (|error| < 4.5e-4), then three Halley steps on
// f(x) = Phi(x) - u, f'' / f' = -x:  s = f / phi(x),  x <- x - s / (1 + s x / 2).  The error is cubed per step with a constant
// x^2 / 12 + 1 / 6 (4.5e-4 -> 2e-10 -> below rounding), so the third step is the polish and what is left is the error of the
// residual f.  That is taken without cancellation: 0.5 erfc(-x / sqrt2) - u in the tail (the subtraction of two nearly equal
// numbers is exact, the error is erfc's relative one, and in x it is that over |x| M(x), M the Mills ratio phi / Phi), and
// (1/2 - u) - 0.5 erf(-x / sqrt2) for u >= 1/4 (1/2 - u is exact there, and erf keeps its relative accuracy as x -> 0, so
// the result is good RELATIVE to x down to x = 0).  Below u = 1e-290 erfc runs out of normal numbers and the same steps are
// taken on log Phi(x) - log u with aq_log_ndtr and the Mills ratio.
#define AQ_SQRT_2PI 2.50662827463100050241576528481105
AQ_HD double aq_ndtri(double u) {
  if (!(u > 0.0) || u > 0.5) return u == 0.0 ? -INFINITY : NAN;
  if (u == 0.5) return 0.0;
  const double lu = log(u);
  const double t = sqrt(-2.0 * lu);
  double x = (2.515517 + t * (0.802853 + t * 0.010328)) / (1.0 + t * (1.432788 + t * (0.189269 + t * 0.001308))) - t;
  if (u < 1e-290) {
    for (int it = 0; it < 3; it++) {
      const double lp = aq_log_ndtr(x);
      const double f = lp - lu;
      const double M = exp(-0.5 * x * x - AQ_LOG_SQRT_2PI - lp);
      x -= f / (M + 0.5 * f * (x + M));
    }
    return x;
  }
  const bool mid = u >= 0.25;
  const double d = 0.5 - u;
  for (int it = 0; it < 3; it++) {
    const double z = -x * AQ_INV_SQRT2;
    const double f = mid ? d - 0.5 * erf(z) : 0.5 * erfc(z) - u;
    const double s = f * (AQ_SQRT_2PI * exp(0.5 * x * x));
    x -= s / (1.0 + 0.5 * s * x);
  }
  return x;
}

// The same function with a short dependency chain, for the sequential SNP recursion where every dependent fp64
// operation costs ~10 ns per SNP and trait tile: exp(-|x|) by a two-step Cody-Waite reduction and a degree-12
// Taylor polynomial in Estrin form (depth 4 instead of 11), the reciprocal of 1 + e in [1, 2] by v_rcp_f64 and two
// Newton steps (no div_scale / div_fixup needed in that range).  21 dependent operations per SNP instead of 36;
// relative error <= 3e-16 (tests/test_special.py).
AQ_HD double aq_exp_neg_fast(double ax) {   // exp(-ax) for ax >= 0
  ax = fmin(ax, 800.0);                     // exp(-800) = 0 in fp64; keeps the reduction finite for any input
  const double k = rint(ax * -1.44269504088896340736);
  double r = fma(k, -6.93147180369123816490e-01, -ax);
  r = fma(k, -1.90821492927058770002e-10, r);
  const double r2 = r * r;
  const double p01 = 1.0 + r;
  const double p23 = fma(r, 1.0 / 6.0, 0.5);
  const double p45 = fma(r, 1.0 / 120.0, 1.0 / 24.0);
  const double p67 = fma(r, 1.0 / 5040.0, 1.0 / 720.0);
  const double p89 = fma(r, 1.0 / 362880.0, 1.0 / 40320.0);
  const double pAB = fma(r, 1.0 / 39916800.0, 1.0 / 3628800.0);
  const double r4 = r2 * r2;
  const double q0 = fma(p23, r2, p01);
  const double q1 = fma(p67, r2, p45);
  const double q2 = fma(pAB, r2, p89);
  const double r8 = r4 * r4;
  const double s0 = fma(q1, r4, q0);
  const double s1 = fma(1.0 / 479001600.0, r4, q2);
  return ldexp(fma(s1, r8, s0), (int)k);
}
// 1/d for a positive normal d: v_rcp_f64 plus two Newton steps on the device (no div_scale / div_fixup sequence), the
// plain quotient on the host.
AQ_HD double aq_recip_pos(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  double y = __builtin_amdgcn_rcp(d);
  y = fma(fma(-d, y, 1.0), y, y);
  y = fma(fma(-d, y, 1.0), y, y);
  return y;
#else
  return 1.0 / d;
#endif
}

// erfcx(z) = exp(z^2) erfc(z) for z >= 0: the degree-24 Chebyshev fit in t = 4/(4+z) (coefficients from
// tools/gen_erfcx_cheb.py, truncation 4e-18 relative), evaluated in the monomial basis of y = 2t - 1 as two interleaved
// Horner chains in y^2 (even and odd powers): 26 fused operations with a dependent chain of 14, against 48 operations and
// a chain of 48 for the Clenshaw recurrence, and slightly more accurate (the monomial coefficients decay like the
// Chebyshev ones, sum |a_m| = 1.0003).  No exponential, no branch, no underflow for any z -- which is why the probit
// terms are built on it rather than on erfc.
AQ_HD double aq_erfcx_pos(double z) {
  const double a[AQ_ERFCX_NCOEF] = {AQ_ERFCX_MONO};
  const double t = 4.0 * aq_recip_pos(4.0 + z);
  const double y = fma(2.0, t, -1.0);
  const double y2 = y * y;
  double pe = a[24], po = a[23];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int j = 22; j >= 0; j -= 2) {
    pe = fma(pe, y2, a[j]);
    if (j >= 1) po = fma(po, y2, a[j - 1]);
  }
  return t * fma(po, y, pe);
}

// log(x) for a positive NORMAL x (no zero / subnormal / inf / nan handling: the one caller guards its argument):
// x = 2^e m, m in [sqrt(1/2), sqrt 2); log m = 2 atanh(s), s = (m - 1)/(m + 1), |s| <= 0.1716, odd series to s^21.
// 30 operations instead of the ~60 of the library log with its special-case handling; error <= 1 ulp of the result or
// 1e-17 absolute near x = 1.
AQ_HD double aq_log_pos(double x) {
  long long b;
  __builtin_memcpy(&b, &x, 8);
  int e = (int)((b >> 52) & 0x7ff) - 1023;
  b = (b & 0x000fffffffffffffLL) | 0x3ff0000000000000LL;
  double m;
  __builtin_memcpy(&m, &b, 8);
  if (m > 1.4142135623730951) { m *= 0.5; e += 1; }
  const double f = m - 1.0;
  const double s = f * aq_recip_pos(2.0 + f);
  const double z = s * s;
  double p = 2.0 / 21.0;
  p = fma(p, z, 2.0 / 19.0);
  p = fma(p, z, 2.0 / 17.0);
  p = fma(p, z, 2.0 / 15.0);
  p = fma(p, z, 2.0 / 13.0);
  p = fma(p, z, 2.0 / 11.0);
  p = fma(p, z, 2.0 / 9.0);
  p = fma(p, z, 2.0 / 7.0);
  p = fma(p, z, 2.0 / 5.0);
  p = fma(p, z, 2.0 / 3.0);
  const double lm = fma(p * z, s, 2.0 * s);                 // log m
  const double de = (double)e;
  return fma(de, 6.93147180369123816490e-01, fma(de, 1.90821492927058770002e-10, lm));
}

// Everything the probit link needs at one point x, from ONE erfcx, ONE exp, ONE log and ONE log1p:
//   lP = log Phi(x), l1 = log(1 - Phi(x))                     pnorm(x, log.p = TRUE), lower / upper tail
//   imr1 = phi(x)/Phi(x), imr0 = -phi(x)/(1 - Phi(x))         inv_mills_ratio_, R/utils.R:172-191 (with its clamps)
// With w = erfcx(|x|/sqrt2) and E = exp(-x^2/2): the far tail is e = w E / 2, so
//   log e = log(w/2) - x^2/2 (no cancellation, no underflow),  log(1 - e) = log1p(-e),
//   phi/e = sqrt(2/pi)/w,  phi/(1 - e) = E / (sqrt(2 pi) (1 - e)).
AQ_HD void aq_probit_terms(double x, double *lP, double *l1, double *imr1, double *imr0) {
  const double w = aq_erfcx_pos(fabs(x) * AQ_INV_SQRT2);
  const double hx2 = 0.5 * x * x;
  const double hx2_lo = 0.5 * fma(x, x, -(x * x));     // x^2/2 = hx2 + hx2_lo exactly: keeps E good to an ulp at |x| ~ 37
  const double E = exp(-hx2) * (1.0 - hx2_lo);
  const double e = 0.5 * w * E;
  const double far_ = log(0.5 * w) - hx2;
  const double near_ = log1p(-e);
  const double rf = AQ_SQRT_2_OVER_PI / w;
  const double rn = (AQ_INV_SQRT_2PI * E) / (1.0 - e);
  double i1, i0;
  if (x > 0.0) { *lP = near_; *l1 = far_; i1 = rn; i0 = -rf; }
  else { *lP = far_; *l1 = near_; i1 = rf; i0 = -rn; }
  if (i1 < -x) i1 = -x;     // R/utils.R:180-181
  if (i0 > -x) i0 = -x;     // R/utils.R:188-189
  *imr1 = i1;
  *imr0 = i0;
}

// The pre-pass form of the same quantities with one log fewer and two divisions fewer:
//   A = log(1 - Phi(x)) - log Phi(x) = +-(log(w / (2 (1 - e))) - x^2/2),  the Mills ratios, and the far tail e
// (log(1 - e) = log1p(-e) recovers the individual tails where the ELBO needs them: near = log1p(-e), far = near -+ A).
AQ_HD void aq_probit_A_imr(double x, double *A, double *imr1, double *imr0, double *e_out) {
  const double w = aq_erfcx_pos(fabs(x) * AQ_INV_SQRT2);
  const double hx2 = 0.5 * x * x;
  const double hx2_lo = 0.5 * fma(x, x, -(x * x));
  const double E = aq_exp_neg_fast(hx2) * (1.0 - hx2_lo);
  const double e = 0.5 * w * E;
  const double om = 1.0 - e;
  const double r = aq_recip_pos(w * om);
  const double inv_w = r * om, inv_om = r * w;
  const double rf = AQ_SQRT_2_OVER_PI * inv_w;
  const double rn = (AQ_INV_SQRT_2PI * E) * inv_om;
  // 0.5 w / (1 - e) lies in (0, 1] and is normal for every |x| whose square is finite (w ~ 1/|x|); the clamp only keeps
  // aq_log_pos inside its domain beyond that, where x^2/2 = inf decides the result anyway
  const double Apos = aq_log_pos(fmax(0.5 * w * inv_om, 1e-300)) - hx2;     // log(e / (1 - e))
  double i1, i0;
  if (x > 0.0) { *A = Apos; i1 = rn; i0 = -rf; }
  else { *A = -Apos; i1 = rf; i0 = -rn; }
  if (i1 < -x) i1 = -x;
  if (i0 > -x) i0 = -x;
  *imr1 = i1;
  *imr0 = i0;
  *e_out = e;
}

// The same three quantities from tables (aq_probit_tab.h, tools/gen_probit_tab.py): A, b = imr1 - imr0 and imr0 are smooth
// functions of ONE variable, so on |x| < AQ_PT_R they are piecewise polynomials of degree AQ_PT_DEG in the local variable of
// an interval of width 1/2 -- three Horner chains (~45 fp64 operations) instead of the ~200 of erfcx + exp + log + reciprocal.
//   A(x) odd;  b(x) = M(x) + M(-x) even;  d(x) = M(x) - M(-x) odd, M = phi / (1 - Phi);  imr0 = -M(x) = -(b + d) / 2.
// `tab` = the table as [3][AQ_PT_DEG + 1][AQ_PT_NI] (the kernels pass their LDS copy: coefficient-major, lanes in different
// intervals hit different banks).  The reference's clamps (R/utils.R:180-181, 188-189: imr1 >= -x, imr0 <= -x) hold strictly
// for the exact functions (M(x) > x) and by a margin >= 1/(2 R) inside the tables.
#if defined(__HIPCC__)
__device__ static const double aq_pt_dev[AQ_PT_LEN] = {AQ_PT_VALUES};
#endif
static const double aq_pt_host[AQ_PT_LEN] = {AQ_PT_VALUES};
AQ_HD const double *aq_pt_table() {
#if defined(__HIP_DEVICE_COMPILE__)
  return aq_pt_dev;
#else
  return aq_pt_host;
#endif
}
// Beyond the tables, |x| >= AQ_PT_R = 12: the far tail is Phi(-v) = phi(v) / v * S(1 / v^2) with the asymptotic series
// S(w) = sum_n (-1)^n (2n - 1)!! w^n, whose terms still fall until n ~ v^2 / 2 = 72: cut after n = 14 the error is below
// 2e-17 relative at v = 12 and shrinks with v.  The near tail 1 - Phi(-v) differs from 1 by less than 2e-33, so
//   M(v) = v / S,   M(-v) = phi(v) / Phi(v) < 3e-32 (nothing next to M(v) >= 12: taken as 0),
//   A = -+ (v^2 / 2 + log v + log sqrt(2 pi) - log S).
// No exponential, a handful of constants: this is what the sweep kernel carries for the rare block that leaves the tables.
AQ_HD void aq_probit_tail(double x, double *A, double *b, double *d) {
  const double v = fabs(x);
  const double w = 1.0 / (v * v);
  double S = 213458046676875.0;
  S = fma(S, w, -7905853580625.0);
  S = fma(S, w, 316234143225.0);
  S = fma(S, w, -13749310575.0);
  S = fma(S, w, 654729075.0);
  S = fma(S, w, -34459425.0);
  S = fma(S, w, 2027025.0);
  S = fma(S, w, -135135.0);
  S = fma(S, w, 10395.0);
  S = fma(S, w, -945.0);
  S = fma(S, w, 105.0);
  S = fma(S, w, -15.0);
  S = fma(S, w, 3.0);
  S = fma(S, w, -1.0);
  S = fma(S, w, 1.0);
  const double M = v * aq_recip_pos(S);                       // S in (0.993, 1]
  const double Apos = aq_log_pos(S) - (0.5 * v * v + AQ_LOG_SQRT_2PI + aq_log_pos(v));   // log Phi(-v) - log Phi(v)
  const bool neg = x < 0.0;
  *A = neg ? -Apos : Apos;
  *b = M;
  *d = neg ? -M : M;
}
// which: bit 0 = A wanted, bit 1 = b and d wanted (annealed sweeps take A at u and the Mills ratios at sqrt(c) u).
// Inside the tables the polynomials, beyond them (and for NaN) aq_probit_tail: any x.
template <int WHICH = 3, class T>
AQ_HD void aq_probit_tab_eval(double x, const T *tab, double *A, double *b, double *d) {
  const double v = fabs(x);
  const double t = v * (1.0 / AQ_PT_W);
  const bool inside = v < AQ_PT_R;            // false for NaN as well
  const int i = (int)fmin(t, (double)(AQ_PT_NI - 1));   // (clamped: the reads stay inside the table for any x)
  const double xl = inside ? fma(2.0, t - (double)i, -1.0) : 0.0;
  const T *p = tab + i;
  constexpr int S = AQ_PT_NI, F = (AQ_PT_DEG + 1) * AQ_PT_NI;
  double pa = 0.0, pb = 0.0, pd = 0.0;
  if (WHICH & 1) pa = p[AQ_PT_DEG * S];
  if (WHICH & 2) { pb = p[F + AQ_PT_DEG * S]; pd = p[2 * F + AQ_PT_DEG * S]; }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = AQ_PT_DEG - 1; k >= 0; k--) {
    if (WHICH & 1) pa = fma(pa, xl, p[k * S]);
    if (WHICH & 2) { pb = fma(pb, xl, p[F + k * S]); pd = fma(pd, xl, p[2 * F + k * S]); }
  }
  const bool neg = x < 0.0;
  double tA = 0.0, tb = 0.0, td = 0.0;
  if (!inside) aq_probit_tail(x, &tA, &tb, &td);
  if (WHICH & 1) *A = inside ? (neg ? -pa : pa) : tA;
  if (WHICH & 2) { *b = inside ? pb : tb; *d = inside ? (neg ? -pd : pd) : td; }
}
// A, imr1, imr0 as aq_probit_A_imr returns them, from the tables where they reach and from the tail series beyond
AQ_HD void aq_probit_A_imr_tab(double x, const double *tab, double *A, double *imr1, double *imr0) {
  double b, d;
  aq_probit_tab_eval<3>(x, tab, A, &b, &d);
  const double m = 0.5 * (b + d);            // M(x)
  *imr0 = -m;
  *imr1 = b - m;                             // M(-x)
}

// log Phi(x) and log(1 - Phi(x)) from the tables (the ELBO pass: R/elbo.R:10-34 reads both for every entry): tabA = the A part of
// aq_pt_table(), tabN = aq_ptn_table() (N(v) = log Phi(v), v >= 0).  Beyond the tables the near side is -Phi(-v) > -2e-33: zero
// next to the far side's <= -72, which the tail series gives.
#if defined(__HIPCC__)
__device__ static const double aq_ptn_dev[AQ_PT_N_LEN] = {AQ_PT_N_VALUES};
#endif
static const double aq_ptn_host[AQ_PT_N_LEN] = {AQ_PT_N_VALUES};
AQ_HD const double *aq_ptn_table() {
#if defined(__HIP_DEVICE_COMPILE__)
  return aq_ptn_dev;
#else
  return aq_ptn_host;
#endif
}
template <class T>
AQ_HD void aq_log_ndtr_pair_tab(double x, const T *tabA, const T *tabN, double *lP, double *l1) {
  const double v = fabs(x);
  const double t = v * (1.0 / AQ_PT_W);
  const bool inside = v < AQ_PT_R;            // false for NaN as well
  const int i = (int)fmin(t, (double)(AQ_PT_NI - 1));
  const double xl = inside ? fma(2.0, t - (double)i, -1.0) : 0.0;
  const T *pA = tabA + i, *pN = tabN + i;
  constexpr int S = AQ_PT_NI;
  double pa = pA[AQ_PT_DEG * S], pn = pN[AQ_PT_DEG * S];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = AQ_PT_DEG - 1; k >= 0; k--) {
    pa = fma(pa, xl, pA[k * S]);
    pn = fma(pn, xl, pN[k * S]);
  }
  double Apos = pa, near_ = pn;               // A(v) = log Phi(-v) - log Phi(v) <= 0, N(v) = log Phi(v)
  if (!inside) {
    double tb, td;
    aq_probit_tail(v, &Apos, &tb, &td);
    near_ = (v != v) ? v : 0.0;              // (NaN stays NaN on both sides)
  }
  const double far_ = near_ + Apos;           // log Phi(-v)
  *lP = x > 0.0 ? near_ : far_;
  *l1 = x > 0.0 ? far_ : near_;
}

// log Phi(x) and log(1 - Phi(x)) = log Phi(-x) together.
AQ_HD void aq_log_ndtr_pair(double x, double *lP, double *l1) {
  double i1, i0;
  aq_probit_terms(x, lP, l1, &i1, &i0);
}

// exp(-log(1+exp(x))) evaluated as the reference's logOnePlusExp does its case
// split (m = max(x,0)): x < 0 -> 1/(1+e^x); x >= 0 -> e^-x/(1+e^-x).
AQ_HD double aq_sigmoid_neg(double x) {
  double e = exp(-fabs(x));
  double num = (x < 0.0) ? 1.0 : e;
  return num / (1.0 + e);
}

// exp(-log(1+exp(x))) with the short chain (see aq_exp_neg_fast above).
AQ_HD double aq_sigmoid_neg_fast(double x) {
  const double e = aq_exp_neg_fast(fabs(x));
  const double d = 1.0 + e;
#if defined(__HIP_DEVICE_COMPILE__)
  double y = __builtin_amdgcn_rcp(d);
  y = fma(fma(-d, y, 1.0), y, y);
  y = fma(fma(-d, y, 1.0), y, y);
#else
  const double y = 1.0 / d;
#endif
  return ((x < 0.0) ? 1.0 : e) * y;
}

// digamma for x > 0: upward recurrence to x >= 10, then the asymptotic series.
AQ_HD double aq_digamma(double x) {
  if (!(x > 0.0)) return NAN;          // the path only calls it with positive arguments; never loop on garbage
  double acc = 0.0;
  for (int i = 0; i < 10 && x < 10.0; i++) {   // at most 10 steps for x > 0
    acc -= 1.0 / x;
    x += 1.0;
  }
  double ix = 1.0 / x, ix2 = ix * ix;
  // B2/2=1/12, B4/4=-1/120, B6/6=1/252, B8/8=-1/240, B10/10=1/132, B12/12=-691/32760, B14/14=1/12
  double ser = ix2 * (1.0 / 12.0 - ix2 * (1.0 / 120.0 - ix2 * (1.0 / 252.0 - ix2 * (1.0 / 240.0 - ix2 * (1.0 / 132.0
               - ix2 * (691.0 / 32760.0 - ix2 * (1.0 / 12.0)))))));
  return acc + log(x) - 0.5 * ix - ser;
}

// E1(x) for 0 < x <= 1: -gamma - ln x - sum_{k>=1} (-x)^k / (k k!)
AQ_HD double aq_expint_e1_small(double x) {
  double sum = 0.0, term = 1.0;
  for (int k = 1; k <= 30; k++) {
    term *= -x / (double)k;
    sum += term / (double)k;
    if (fabs(term) < 1e-18 * fabs(sum)) break;
  }
  return -AQ_EULER_GAMMA - log(x) - sum;
}

// One element's modified-Lentz state for exp(x) E1(x), x > 1, exactly as the
// reference iterates it (R/utils.R:392-419): eps1 = 1e-30.  step(j) performs the
// body for iteration counter j (the reference increments j first, so the first
// call is j = 2) and returns |Delta - 1|.
struct AqLentz {
  double f, C, D;
};
AQ_HD void aq_lentz_init(AqLentz *s) {
  s->f = 1e-30;
  s->C = 1e-30;
  s->D = 0.0;
}
AQ_HD double aq_lentz_step(AqLentz *s, double x, int j) {
  double jm1sq = (double)(j - 1) * (double)(j - 1);
  double Dc = x + 2.0 * j - 1.0 - jm1sq * s->D;
  double Cc = x + 2.0 * j - 1.0 - jm1sq / s->C;
  Dc = 1.0 / Dc;
  double Delta = Cc * Dc;
  s->f = s->f * Delta;
  s->C = Cc;
  s->D = Dc;
  return fabs(Delta - 1.0);
}
AQ_HD double aq_lentz_finish(const AqLentz *s, double x) { return 1.0 / (x + 1.0 + s->f); }

// Unnormalised upper incomplete gamma Gamma(a, x) for 0 < a < 2, x > 0.
//   x >= 1 : modified-Lentz continued fraction (Numerical-Recipes form), relative 1e-16
//   x <  1 : Gamma(a,1) + int_x^1 t^(a-1) e^-t dt, the integral as the alternating
//            series sum_k (-1)^k/k! (1 - x^(a+k))/(a+k), first term via expm1 so a -> 0 is safe
AQ_HD double aq_gamma_inc_cf(double a, double x) {
  const double tiny = 1e-300;
  double b = x + 1.0 - a;
  double c = 1.0 / tiny;
  double d = 1.0 / b;
  double h = d;
  for (int i = 1; i <= 500; i++) {
    double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < 1e-16) break;
  }
  return exp(-x + a * log(x)) * h;
}
AQ_HD double aq_gamma_inc_upper(double a, double x) {
  if (x >= 1.0) return aq_gamma_inc_cf(a, x);
  double g1 = aq_gamma_inc_cf(a, 1.0);
  double lx = log(x);
  double sum = 0.0, sgn_over_fact = 1.0;
  for (int k = 0; k <= 40; k++) {
    double ak = a + (double)k;
    double t = sgn_over_fact * (-expm1(ak * lx)) / ak;
    sum += t;
    if (k > 0 && fabs(t) < 1e-18 * fabs(sum)) break;
    sgn_over_fact *= -1.0 / (double)(k + 1);
  }
  return g1 + sum;
}

// Kummer's M(a; b; x) = 1F1 by its power series, for x > 0 and b not a non-positive integer (gsl::hyperg_1F1 at the call sites of
// update_annealed_lam2_inv_vb_, R/update_vb.R:78-81: b in {3 - c, 2 - c, c, c - 1} with 0 < c < 1, so b = c - 1 is negative and not
// an integer; every term after the first then has one sign).  Terms grow until k ~ x: good for the L of the path (order one);
// beyond x ~ 700 it overflows as the reference's own expression does.
AQ_HD double aq_hyp1f1_series(double a, double b, double x) {
  double term = 1.0, sum = 1.0;
  for (int k = 0; k < 4000; k++) {
    term *= (a + k) / (b + k) * x / (double)(k + 1);
    sum += term;
    if (fabs(term) < 1e-17 * fabs(sum) && (double)k > x) break;
  }
  return sum;
}
// update_annealed_lam2_inv_vb_(L_vb, c, df) for df != 1 exactly as the reference writes it (R/update_vb.R:76-81): a quotient of two
// differences of Kummer functions -- Gamma(a + 1) U(a + 1, 3 - c, L) / (Gamma(a) U(a, 2 - c, L)) / df with a = c (df - 1) / 2 + 1 in
// Tricomi's U -- which cancels as L grows (the two terms of each difference grow like e^L, the difference falls like L^-a).
// Reproduced term by term, not repaired: parity with the reference is the contract.
AQ_HD double aq_annealed_lam2_inv_df(double L, double c, double df) {
  const double a = c * (df - 1.0) / 2.0 + 1.0, ap = c * (df + 1.0) / 2.0;
  const double gc = tgamma(c), gap = tgamma(ap);
  const double num = tgamma(a + 1.0) * gc * aq_hyp1f1_series(a + 1.0, 3.0 - c, L) / (c - 1.0) / (c - 2.0) / gap +
                     tgamma(2.0 - c) * pow(L, c - 2.0) * aq_hyp1f1_series(ap, c - 1.0, L);
  const double den = tgamma(a) * gc * aq_hyp1f1_series(a, 2.0 - c, L) / (c - 1.0) / gap +
                     tgamma(1.0 - c) * pow(L, c - 1.0) * aq_hyp1f1_series(ap, c, L);
  return num / den / df;
}

// Inverse Mills ratios and the probit auxiliary mean Z of one (j,k) entry,
// R/update_vb.R:217-234 with R/utils.R:172-191.  U = sqrt_c*u, lP = log Phi(U), l1 = log(1-Phi(U)).
AQ_HD double aq_probit_z(double gam, double u, double U, double lP, double l1, double sqrt_c) {
  double base = -0.5 * U * U - AQ_LOG_SQRT_2PI;
  double imr1 = exp(base - lP);
  if (imr1 < -U) imr1 = -U;
  double imr0 = -exp(base - l1);
  if (imr0 > -U) imr0 = -U;
  return (gam * (imr1 - imr0) + imr0) / sqrt_c + u;
}

// log(sum(exp(x))) as log_sum_exp_ writes it (R/utils.R:194-203: offset = min(x) if max |x| > max x, else max(x)).
AQ_HD double aq_log_sum_exp(const double *x, int n) {
  double mx = x[0], mn = x[0], ma = fabs(x[0]);
  for (int i = 1; i < n; i++) { mx = fmax(mx, x[i]); mn = fmin(mn, x[i]); ma = fmax(ma, fabs(x[i])); }
  const double off = ma > mx ? mn : mx;
  double s = 0.0;
  for (int i = 0; i < n; i++) s += exp(x[i] - off);
  return log(s) + off;
}

// compute_integral_hs_ (R/utils.R:425-568): int_0^inf x^n (1 + alpha x)^-m exp(-beta x) dx, Q = exp(beta/alpha) E1(beta/alpha),
// for the (m, n) the horseshoe with df = 5 and 7 asks for -- (3,3), (3,2), (4,4), (4,3) -- term by term as the reference sums
// them (differences of exp(log_sum_exp) of the positive and the negative terms: digits are lost as beta / alpha grows, and
// the reference's n = 4 list does not add up to the integral at all -- the quadrature test under tests/; both are reproduced, not repaired).
AQ_HD double aq_hs_integral(double alpha, double beta, int m, int n, double Q) {
  const double la = log(alpha), lb = log(beta), lQ = log(Q);
  const double l2 = 0.6931471805599453, l3 = 1.0986122886681098, l4 = 1.3862943611198906, l6 = 1.791759469228055;
  double v1[8], v2[8];
  int n1 = 0, n2 = 0;
  if (m == 3 && n == 3) {                       // :446-458
    v1[n1++] = -3 * la - lb; v1[n1++] = l3 - 4 * la; v1[n1++] = -5 * la - l2 + lb;
    v2[n2++] = l3 - 4 * la + lQ; v2[n2++] = l3 - 5 * la + lb + lQ; v2[n2++] = -4 * la - l2; v2[n2++] = -6 * la - l2 + 2 * lb + lQ;
  } else if (m == 4 && n == 4) {                // :460-474
    v1[n1++] = -4 * la - lb; v1[n1++] = l4 - 5 * la; v1[n1++] = l2 - 5 * la; v1[n1++] = l2 - 7 * la + 2 * lb + lQ;
    v1[n1++] = -7 * la - l6 + 2 * lb; v1[n1++] = -5 * la - l3;
    v2[n2++] = l4 - 5 * la + lQ; v2[n2++] = l4 - 6 * la + lb + lQ; v2[n2++] = l2 - 7 * la + lb; v2[n2++] = -6 * la - l6 + lb;
  } else if (m == 3 && n == 2) {                // :516-530
    v1[n1++] = -3 * la + lQ; v1[n1++] = -3 * la - l2; v1[n1++] = -5 * la - l2 + 2 * lb + lQ; v1[n1++] = -4 * la + l2 + lb + lQ;
    v2[n2++] = -4 * la - l2 + lb; v2[n2++] = -3 * la + l2;
  } else if (m == 4 && n == 3) {                // :532-560, the general m = n + 1 lists written out for n = 3 (lfactorial(3) = log 6)
    v1[n1++] = -4 * la + lQ;                                   // -(n+1) log a + log Q
    v1[n1++] = -7 * la - l6 + lb + 2 * la;                     // j = 2: lfactorial(1) + (3-2) log b + 2 log a
    v1[n1++] = -7 * la - l6 + 3 * lb + lQ;
    v1[n1++] = -3 * la + l3 - 3 * la - l2 + 2 * la;            // k = 2, j = 2
    v1[n1++] = -3 * la + l3 - 2 * la + lb + lQ;                // k = 1: -(1+k) log a - lfactorial(k) + k log b + log Q
    v1[n1++] = -3 * la + l3 - 3 * la - l2 + 2 * lb + lQ;       // k = 2
    v2[n2++] = -7 * la - l6 + 2 * lb + la;                     // j = 1: lfactorial(0) + (3-1) log b + log a
    v2[n2++] = -7 * la - l6 + l2 + 3 * la;                     // j = 3: lfactorial(2) + 0 + 3 log a
    v2[n2++] = -3 * la + l3 - 2 * la + la;                     // k = 1, j = 1
    v2[n2++] = -3 * la + l3 - 3 * la - l2 + lb + la;           // k = 2, j = 1
  } else {
    return NAN;
  }
  return exp(aq_log_sum_exp(v1, n1)) - exp(aq_log_sum_exp(v2, n2));
}

