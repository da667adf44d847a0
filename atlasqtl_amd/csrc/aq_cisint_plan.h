// aq_cisint_plan.h -- the launch plan of the interaction cis scan (aq_prep_cis_int; kernels in aq_cisint_kernels.h): the plan of
// aq_cis_plan.h for the same windows (complete Y, no permutations: the order of the traits, the trait tiles and the work items
// are taken over unchanged), and on top of it what the interaction adds: the two matrix-instruction streams of the tile kernel
// fed from one staged panel of Xs, the number of basis vectors, the static LDS of the tile kernel, the length of the
// zero-padded copy of the multiplier, and the bytes of the residual traits Yo [q_active][n], of the per-predictor arrays and of
// the basis with the multiplier.  A pure function in the manner of aq_cis_plan.h: integer arithmetic only, no HIP call, no
// getenv.  aq_prep_cis_int runs it before it allocates anything; aq_cisint_plan_query exposes it on the C ABI without a device.
// The checks of the basis and of the multiplier are here too: they are host arithmetic.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "aq_cis_plan.h"

#define AQ_CISINT_NB_MAX 256                 // basis vectors: the trait kernel holds one dot product each in LDS
#define AQ_CISINT_ORTHO_TOL 1e-8             // max |B'B - I|
#define AQ_CISINT_SPAN_TOL 1e-10             // |m - B B'm|^2 <= this |m|^2
#define AQ_CISINT_PANEL_MAX (4ll << 30)      // bytes of Yo

// static LDS of a workgroup of aq_k_ci_tile: the panel of X and the one trait-side panel (the residual traits), rows of
// AQ_MSCREEN_STR doubles; the two columns of per-trait candidates (double r, int snp); per trait S'yy_t, the cutoff, the floor
// of S'' (1e-10 S0yy_t), whether the trait can be tested, s_lo, s_hi and the trait's own index
AQ_MSCREEN_HD constexpr int aq_cisint_lds_bytes() {
  return 2 * AQ_CIS_TILE * AQ_MSCREEN_STR * 8 + 2 * AQ_CIS_TILE * (8 + 4) + AQ_CIS_TILE * (8 + 8 + 8 + 4 + 4 + 4 + 4);
}

// the doubles of the zero-padded copy of the multiplier: n rounded up to whole sample chunks, so that the tile kernel reads
// the multiplier of every staged sample without a guard
AQ_MSCREEN_HD constexpr long long aq_cisint_mult_pad(int n) {
  return ((long long)n + AQ_MSCREEN_NC - 1) / AQ_MSCREEN_NC * AQ_MSCREEN_NC;
}

// n_basis in [1, AQ_CISINT_NB_MAX]: below it is no basis at all (AQ_ERR_ARG), above it more than the kernels hold
// (AQ_ERR_UNSUPPORTED)
static inline int aq_cisint_check_nb(int n_basis, const char *who, std::string *err) {
  if (n_basis < 1) {
    if (err) *err = std::string(who) + ": n_basis >= 1 required, " + std::to_string(n_basis) + " given";
    return AQ_ERR_ARG;
  }
  if (n_basis > AQ_CISINT_NB_MAX) {
    if (err)
      *err = std::string(who) + ": " + std::to_string(n_basis) + " basis vectors are not supported, at most " +
             std::to_string(AQ_CISINT_NB_MAX) + " are";
    return AQ_ERR_UNSUPPORTED;
  }
  return AQ_OK;
}

// basis: [n_basis][n], mult: n doubles.  In this order: a non-finite entry of basis or of mult; max |B'B - I| >
// AQ_CISINT_ORTHO_TOL; |m - B B'm|^2 > AQ_CISINT_SPAN_TOL |m|^2; mult all zero.  Long double sums: the check does not depend on
// the order of the samples.
static inline int aq_cisint_check_basis(const double *basis, int n_basis, const double *mult, int n, const char *who, std::string *err) {
  const std::string w(who);
  const size_t nn = (size_t)n;
  for (size_t i = 0; i < (size_t)n_basis * nn; i++)
    if (!std::isfinite(basis[i])) {
      if (err) *err = w + ": basis vector " + std::to_string(i / nn) + " has a non-finite entry";
      return AQ_ERR_ARG;
    }
  for (size_t i = 0; i < nn; i++)
    if (!std::isfinite(mult[i])) {
      if (err) *err = w + ": mult[" + std::to_string(i) + "] is not finite";
      return AQ_ERR_ARG;
    }
  for (int a = 0; a < n_basis; a++)
    for (int b = 0; b <= a; b++) {
      long double s = 0.0L;
      for (size_t i = 0; i < nn; i++) s += (long double)basis[(size_t)a * nn + i] * basis[(size_t)b * nn + i];
      const long double dev = fabsl(s - (a == b ? 1.0L : 0.0L));
      if (!(dev <= (long double)AQ_CISINT_ORTHO_TOL)) {
        if (err)
          *err = w + ": the basis is not orthonormal: |b_" + std::to_string(a) + "'b_" + std::to_string(b) + " - " + (a == b ? "1" : "0") +
                 "| = " + std::to_string((double)dev) + " exceeds 1e-8";
        return AQ_ERR_ARG;
      }
    }
  std::vector<long double> res(nn);
  long double m2 = 0.0L;
  for (size_t i = 0; i < nn; i++) {
    res[i] = mult[i];
    m2 += (long double)mult[i] * mult[i];
  }
  for (int a = 0; a < n_basis; a++) {
    long double d = 0.0L;
    for (size_t i = 0; i < nn; i++) d += (long double)basis[(size_t)a * nn + i] * mult[i];
    for (size_t i = 0; i < nn; i++) res[i] -= (long double)basis[(size_t)a * nn + i] * d;
  }
  long double r2 = 0.0L;
  for (size_t i = 0; i < nn; i++) r2 += res[i] * res[i];
  if (r2 > (long double)AQ_CISINT_SPAN_TOL * m2) {
    if (err) *err = w + ": mult is not in the span of the basis: the basis must span the intercept, the covariates and the interaction variable";
    return AQ_ERR_ARG;
  }
  if (!(m2 > 0.0L)) {
    if (err) *err = w + ": mult is all zero: the interaction variable is constant";
    return AQ_ERR_ARG;
  }
  return AQ_OK;
}

// work may be NULL (the query).  The windows are checked again here, so that the query refuses what the entry refuses.
static inline int aq_cisint_make_plan(int n, int p1, int q, int ncu, const int32_t *s_lo, const int32_t *s_hi, int n_basis, const char *who,
                                      aq_cisint_plan *pl, aq_cis_work *work, std::string *err) {
  const int rcn = aq_cisint_check_nb(n_basis, who, err);
  if (rcn != AQ_OK) return rcn;
  aq_cis_work local;
  aq_cis_work &wk = work ? *work : local;
  aq_cis_plan cis{};
  const int rc = aq_cis_make_plan(n, p1, q, 0, ncu, s_lo, s_hi, 0, 0, 0, who, &cis, &wk, err);
  if (rc != AQ_OK) return rc;
  const long long panel = 8ll * (wk.q_active > 0 ? wk.q_active : 1) * n;
  if (panel > AQ_CISINT_PANEL_MAX) {
    if (err) *err = std::string(who) + ": the residual traits (" + std::to_string(panel) + " bytes) exceed 4 GiB";
    return AQ_ERR_UNSUPPORTED;
  }
  pl->cis = cis;
  pl->streams = 2;
  pl->n_basis = n_basis;
  pl->lds_bytes = aq_cisint_lds_bytes();
  pl->mult_pad = (int32_t)aq_cisint_mult_pad(n);
  pl->yo_bytes = panel;
  pl->pred_bytes = (long long)p1 * (4 * 8 + 4);
  pl->basis_bytes = 8ll * n_basis * n + 8ll * aq_cisint_mult_pad(n);
  return AQ_OK;
}
