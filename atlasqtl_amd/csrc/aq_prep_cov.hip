// aq_prep_cov.hip -- the covariates of aq_prepare_data_cov / aq_prepare_data_bed_cov / aq_prepare_data_opt
// (include/atlasqtl_hip.h; kernels in aq_cov_kernels.h): the orthonormal basis of [1, Z] on the host (aq_cov_basis), the two
// residual passes on the device that the pipeline of aq_prepare.hip puts in front of its own work on X and on Y, and
// aq_prep_cov_info.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "aq_prep.h"          // aq_prep, the prototypes of what aq_prepare.hip calls here; aq_internal.h
#include "aq_cov_kernels.h"   // aq_k_cov_residualise, aq_k_cov_residualise_y

static int aq_cov_check_dims(int n, int d) {
  if (d < 1 || d > AQ_COV_MAX_D)
    return aq_fail(AQ_ERR_ARG, "covariates: between 1 and " + std::to_string(AQ_COV_MAX_D) + " columns are supported, " +
                                   std::to_string(d) + " given");
  if (n < 2 || d + 1 >= n)
    return aq_fail(AQ_ERR_ARG, "covariates: " + std::to_string(d) + " columns and the intercept need more than " +
                                   std::to_string(d + 1) + " samples, n = " + std::to_string(n));
  return AQ_OK;
}

// Q (n x D column-major, D = d + 1): an orthonormal basis of [1, Z], columns in order, by modified Gram-Schmidt applied twice
// with long double dot products.  Covariate l is collinear when what is left of it after the intercept and the covariates
// before it has a squared norm <= AQ_COV_TOL times its own.
extern "C" int aq_cov_basis(const double *Z, int32_t n, int32_t d, double *Q, int32_t *bad_col) {
  if (bad_col) *bad_col = -1;
  if (!Z || !Q) return aq_fail(AQ_ERR_ARG, "aq_cov_basis: NULL argument");
  AQ_TRY(aq_cov_check_dims(n, d));
  const size_t nd = (size_t)n * d;
  for (size_t i = 0; i < nd; i++)
    if (!std::isfinite(Z[i])) return aq_fail(AQ_ERR_ARG, "covariates must be a numeric matrix, finite without missing value.");
  const double q0 = 1.0 / std::sqrt((double)n);
  for (int i = 0; i < n; i++) Q[i] = q0;
  for (int l = 1; l <= d; l++) {
    double *v = Q + (size_t)l * n;
    const double *z = Z + (size_t)(l - 1) * n;
    long double own = 0.0L;
    for (int i = 0; i < n; i++) { v[i] = z[i]; own += (long double)z[i] * z[i]; }
    for (int pass = 0; pass < 2; pass++)
      for (int k = 0; k < l; k++) {
        const double *qk = Q + (size_t)k * n;
        long double dot = 0.0L;
        for (int i = 0; i < n; i++) dot += (long double)qk[i] * v[i];
        const double c = (double)dot;
        for (int i = 0; i < n; i++) v[i] -= qk[i] * c;
      }
    long double rem = 0.0L;
    for (int i = 0; i < n; i++) rem += (long double)v[i] * v[i];
    if (!(rem > (long double)AQ_COV_TOL * own)) {
      if (bad_col) *bad_col = l - 1;
      return aq_fail(AQ_ERR_ARG, "column " + std::to_string(l) + " of the covariates is collinear with the intercept and the "
                                     "columns before it (a constant column is collinear with the intercept)");
    }
    const double nrm = (double)sqrtl(rem);
    for (int i = 0; i < n; i++) v[i] /= nrm;
  }
  return AQ_OK;
}

// the checks of a covariate argument and its basis, all on the host: Q is n x (d + 1) afterwards
int aq_cov_host_basis(const aq_prep_cov *cov, int n, const char *who, std::vector<double> *Q) {
  if (!cov->Z) return aq_fail(AQ_ERR_ARG, std::string(who) + ": NULL covariate pointer");
  AQ_TRY(aq_cov_check_dims(n, cov->d));
  Q->resize((size_t)n * (cov->d + 1));
  return aq_cov_basis(cov->Z, n, cov->d, Q->data(), nullptr);
}

// x_j <- x_j - Q (Q' x_j) for every column of the device matrix dX into dXr (dX itself for T = double)
template <typename T>
static int aq_cov_residualise_x_of(aq_prep *h, const T *dX, double *dXr, const double *dQt, int D) {
  const int n = h->n, p = h->p;
  AqDev<uint8_t> dabs;
  AqDev<double> dr2;
  AQ_TRY(dabs.alloc((size_t)p));
  AQ_TRY(dr2.alloc((size_t)p));
  hipLaunchKernelGGL((aq_k_cov_residualise<T>), dim3(p), dim3(256), 0, 0, dX, n, D, dQt, dXr, dabs.get(), dr2.get());
  AQ_HIP(hipGetLastError());
  h->n_cov = D - 1;
  h->cov_absorbed.resize(p);
  h->cov_r2.resize(p);
  AQ_HIP(hipMemcpy(h->cov_absorbed.data(), dabs.get(), (size_t)p, hipMemcpyDeviceToHost));
  AQ_HIP(hipMemcpy(h->cov_r2.data(), dr2.get(), (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}

int aq_cov_residualise_x(aq_prep *h, const int8_t *dG, double *dX, const double *dQt, int D) {
  return dG ? aq_cov_residualise_x_of<int8_t>(h, dG, dX, dQt, D) : aq_cov_residualise_x_of<double>(h, dX, dX, dQt, D);
}

int aq_cov_residualise_y(aq_prep *h, const double *dY, const double *dQt, int D, int *dnobs, int *dflag) {
  hipLaunchKernelGGL(aq_k_cov_residualise_y, dim3(h->q), dim3(256), aq_cov_y_lds_bytes(D), 0, dY, h->n, D, dQt, h->Yc.get(), dnobs, dflag);
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

extern "C" int aq_prep_cov_info(aq_prep_handle h, int32_t *d, uint8_t *absorbed, double *r2) {
  if (!h) return aq_fail(AQ_ERR_ARG, "NULL handle");
  if (d) *d = h->n_cov;
  if (absorbed) std::copy(h->cov_absorbed.begin(), h->cov_absorbed.end(), absorbed);
  if (r2) std::copy(h->cov_r2.begin(), h->cov_r2.end(), r2);
  return AQ_OK;
}
