// aq_prepare.hip -- the O(n p) input construction of prepare_data_ on the device:
//   X <- scale(X)                                  R/prepare_atlasqtl.R:57   (centre, divide by the n - 1 standard deviation)
//   rm_constant_   (0/0 = NaN columns)             R/utils.R:276-302
//   rm_collinear_  (duplicated(mat, MARGIN = 2))   R/utils.R:304-343        (later copies of an identical column go)
//   Y <- scale(Y, center = TRUE, scale = FALSE)    R/prepare_atlasqtl.R:83   (column means over the observed entries)
//   and the two missingness guards                 R/prepare_atlasqtl.R:39-45
// X arrives as fp64 or as int8 dosages (0 / 1 / 2 ...: 1 byte per genotype, "block-standardised genotype X" of BASELINE.json
// configs[4]): at C5 that is 1 GB over PCIe instead of 8 GB, and the fp64 matrix never exists on the host.  The result stays
// on the device (compact n x p_kept fp64 + centred Y) and is handed to aq_vb_create as device pointers.
// aq_prepare_data_bed takes the genotypes as a PLINK 1 .bed stores them, 2 bits each: the packed blocks are uploaded (a
// quarter of the int8 bytes) and one decode pass unpacks them into the int8 buffer that the same pipeline then reads.
// All of it is HBM-bound streaming: one read of X for the column statistics, one read + one write for the standardised
// matrix with its column hashes, one gather pass for the compaction.
// aq_prepare_data_cov / aq_prepare_data_bed_cov regress covariates out of X and Y first (aq_cov_kernels.h): the residuals of
// X are formed as fp64 on the device, enter the fp64 pipeline unchanged and are freed once the compact matrix is written.
// aq_prep_ld_prune thins the compact matrix of a finished handle for linkage disequilibrium (aq_ld_kernels.h): the banded
// correlation matrix on the f64 matrix pipe, thresholded into bits, a first-one-wins scan, and a gather of the kept columns.
// aq_prep_grm forms the n x n genetic relationship matrix Xs Xs' / p1 of a finished handle's current matrix on the same pipe
// (aq_grm_kernels.h, planned by aq_grm_plan.h) and copies it to the host.
// aq_prep_grm_apply applies that matrix to a block of vectors without forming it, Xs (Xs' Q) / p1 (aq_pcs_kernels.h, planned by
// aq_pcs_plan.h): the step of subspace iteration for its leading eigenvectors, for any n a handle holds.
// aq_prepare_data_opt is the four aq_prepare_data* entries in one and can put the rank-based inverse normal transform of the
// traits (aq_ytrans_kernels.h, planned by aq_ytrans_plan.h) in front of everything that is done to Y; aq_rank_int is that
// transform alone.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <memory>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>
#include "aq_internal.h"   // aq_fail, AQ_HIP, aq_need_device, AqDev

struct aq_prep {
  int n = 0, p = 0, q = 0, p_kept = 0, device = 0;
  AqDev<double> Xs;   // n x p_kept, standardised, compact
  AqDev<double> Yc;   // n x q, centred (NaN = missing)
  std::vector<uint8_t> bool_cst, bool_coll;   // p each (bool_coll in the ORIGINAL column numbering)
  std::vector<int32_t> dup_of;                // original index of the kept column a removed duplicate equals, else -1
  std::vector<double> mean, sd;               // p each
  std::vector<int32_t> gcounts;               // 4 x p (hom A1, het, hom A2, missing): aq_prepare_data_bed only
  int n_cov = 0;                              // covariates regressed out of X and Y (0: none)
  std::vector<uint8_t> cov_absorbed;          // p: the covariates explain the column (written as 0.0, reported constant)
  std::vector<double> cov_r2;                 // p: share of the column's variance that the covariates explain
  bool ld_done = false;                       // aq_prep_ld_prune has run: Xs holds the kept columns only
  std::vector<uint8_t> ld_removed;            // p: removed by aq_prep_ld_prune (original numbering, like the two below)
  std::vector<int32_t> ld_of;                 // p: original index of the kept column that tags a removed one, else -1
  std::vector<double> ld_r2;                  // p: r^2 of a removed column with its tag, else NaN
  int yt_method = 0;                          // transform of Y before everything else (0: none, 1: rank-based inverse normal)
  double yt_offset = 0.0;                     // its c
  std::vector<int32_t> yt_nobs, yt_ntied;     // q each: observed values of the trait, and those that share their value
};

template <typename T>
__device__ __forceinline__ double aq_xval(const T *X, size_t i) { return (double)X[i]; }

// block-wide sum in a fixed order (tree over 256 threads): deterministic, identical for identical columns
__device__ __forceinline__ double aq_block_sum(double v, double *sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

#include "aq_cov_kernels.h"   // aq_k_cov_residualise, aq_k_cov_residualise_y
#include "aq_ld_kernels.h"    // aq_k_ld_band, aq_k_ld_scan, aq_k_ld_tag_r2, aq_k_ld_gather
#include "aq_grm_kernels.h"   // aq_k_grm_partial, aq_k_grm_reduce; aq_grm_make_plan
#include "aq_pcs_kernels.h"   // aq_k_pcs_pack_q, aq_k_pcs_xtq, aq_k_pcs_xt, aq_k_pcs_reduce, aq_k_pcs_colss; aq_pcs_make_plan
#include "aq_ytrans_kernels.h"   // aq_k_yt_lds, aq_k_yt_global; aq_ytrans_device, aq_ytrans_make_plan

// one workgroup per column: mean (sum / n, then one refinement pass as R's long-double colMeans would give), the n - 1
// standard deviation of the centred values, and whether the column is constant
template <typename T>
__global__ __launch_bounds__(256) void aq_k_col_stats(const T *__restrict__ X, int n, double *__restrict__ mean,
                                                     double *__restrict__ sd, uint8_t *__restrict__ cst) {
  __shared__ double sh[256];
  __shared__ int ne;
  const size_t base = (size_t)blockIdx.x * n;
  const double x0 = aq_xval(X, base);
  if (threadIdx.x == 0) ne = 0;
  __syncthreads();
  double s = 0.0;
  int diff = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double v = aq_xval(X, base + i);
    s += v;
    diff |= (v != x0);
  }
  if (diff) ne = 1;
  double m = aq_block_sum(s, sh) / n;
  double s2 = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s2 += aq_xval(X, base + i) - m;
  m += aq_block_sum(s2, sh) / n;
  const bool is_cst = (ne == 0);
  if (is_cst) m = x0;                       // R centres a constant column to exactly 0 -> 0/0 = NaN -> rm_constant_
  double ss = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double d = aq_xval(X, base + i) - m;
    ss += d * d;
  }
  ss = aq_block_sum(ss, sh);
  if (threadIdx.x == 0) {
    mean[blockIdx.x] = m;
    sd[blockIdx.x] = sqrt(ss / (double)(n - 1));
    cst[blockIdx.x] = is_cst ? 1 : 0;
  }
}

__device__ __forceinline__ unsigned long long aq_mix64(unsigned long long x) {   // splitmix64 finaliser
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// standardised values (x - mean) / sd into the compact matrix (column `dst[j]`, or skipped when dst[j] < 0) and a 128-bit
// position-dependent hash of each column's bit patterns: identical columns -> identical hashes, in any summation order
template <typename T>
__global__ __launch_bounds__(256) void aq_k_standardise(const T *__restrict__ X, int n, const double *__restrict__ mean,
                                                       const double *__restrict__ sd, const int *__restrict__ dst,
                                                       double *__restrict__ Xs, unsigned long long *__restrict__ hash) {
  __shared__ unsigned long long h0[256], h1[256];
  const int j = blockIdx.x;
  const size_t base = (size_t)j * n;
  const double m = mean[j], s = sd[j];
  const int d = dst ? dst[j] : j;
  unsigned long long a = 0, b = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double v = (aq_xval(X, base + i) - m) / s;
    if (d >= 0 && Xs) Xs[(size_t)d * n + i] = v;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    a += aq_mix64(bits + 0x9e3779b97f4a7c15ull * (unsigned long long)(i + 1));
    b += aq_mix64((bits ^ 0xc2b2ae3d27d4eb4full) + 0x165667b19e3779f9ull * (unsigned long long)(i + 1));
  }
  h0[threadIdx.x] = a;
  h1[threadIdx.x] = b;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) { h0[threadIdx.x] += h0[threadIdx.x + st]; h1[threadIdx.x] += h1[threadIdx.x + st]; }
    __syncthreads();
  }
  if (threadIdx.x == 0 && hash) { hash[2 * j] = h0[0]; hash[2 * j + 1] = h1[0]; }
}

// are the standardised columns ja and jb bit-identical?  (confirms a hash match: out[pair] = number of differing entries)
template <typename T>
__global__ __launch_bounds__(256) void aq_k_cols_equal(const T *__restrict__ X, int n, const double *__restrict__ mean,
                                                      const double *__restrict__ sd, const int *__restrict__ pairs,
                                                      int *__restrict__ out) {
  const int ja = pairs[2 * blockIdx.x], jb = pairs[2 * blockIdx.x + 1];
  int diff = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double va = (aq_xval(X, (size_t)ja * n + i) - mean[ja]) / sd[ja];
    const double vb = (aq_xval(X, (size_t)jb * n + i) - mean[jb]) / sd[jb];
    diff += (__double_as_longlong(va) != __double_as_longlong(vb));
  }
  if (diff) atomicAdd(&out[blockIdx.x], diff);
}

// Y <- scale(Y, center = TRUE, scale = FALSE): column means over the observed entries; nobs per column
__global__ __launch_bounds__(256) void aq_k_centre_y(const double *__restrict__ Y, int n, double *__restrict__ Yc,
                                                    int *__restrict__ nobs) {
  __shared__ double sh[256];
  const size_t base = (size_t)blockIdx.x * n;
  double s = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double v = Y[base + i];
    if (v == v) { s += v; c += 1.0; }
  }
  s = aq_block_sum(s, sh);
  c = aq_block_sum(c, sh);
  double m = c > 0 ? s / c : 0.0;
  double s2 = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double v = Y[base + i];
    if (v == v) s2 += v - m;
  }
  if (c > 0) m += aq_block_sum(s2, sh) / c;
  else aq_block_sum(s2, sh);
  for (int i = threadIdx.x; i < n; i += 256) Yc[base + i] = Y[base + i] - m;   // NaN - m = NaN
  if (threadIdx.x == 0) nobs[blockIdx.x] = (int)c;
}

// everything from a device-resident n x p matrix on: column statistics, hashes, duplicate confirmation, compact standardise
template <typename T>
static int aq_prepare_x_device(aq_prep *h, const T *dX) {
  const int n = h->n, p = h->p;
  AqDev<double> dmean_, dsd_;
  AqDev<uint8_t> dcst;
  AqDev<unsigned long long> dhash;
  AqDev<int> ddst, dpairs_, dout_;
  std::vector<unsigned long long> hash((size_t)2 * p);
  std::vector<int> dst(p, -1);
  {
    AQ_TRY(dmean_.alloc((size_t)p));
    AQ_TRY(dsd_.alloc((size_t)p));
    AQ_TRY(dcst.alloc((size_t)p));
    AQ_TRY(dhash.alloc((size_t)2 * p));
    double *const dmean = dmean_.get(), *const dsd = dsd_.get();
    hipLaunchKernelGGL((aq_k_col_stats<T>), dim3(p), dim3(256), 0, 0, dX, n, dmean, dsd, dcst.get());
    // first pass over the standardised values: hashes only (nothing is written yet: the compact column index needs them)
    hipLaunchKernelGGL((aq_k_standardise<T>), dim3(p), dim3(256), 0, 0, dX, n, dmean, dsd, (const int *)nullptr, (double *)nullptr, dhash.get());
    AQ_HIP(hipGetLastError());
    h->bool_cst.assign(p, 0); h->bool_coll.assign(p, 0); h->dup_of.assign(p, -1); h->mean.resize(p); h->sd.resize(p);
    AQ_HIP(hipMemcpy(h->bool_cst.data(), dcst.get(), (size_t)p, hipMemcpyDeviceToHost));
    AQ_HIP(hipMemcpy(h->mean.data(), dmean, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
    AQ_HIP(hipMemcpy(h->sd.data(), dsd, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
    AQ_HIP(hipMemcpy(hash.data(), dhash.get(), hash.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (const char *e = getenv("AQ_PREP_HASH_MASK")) {   // test hook: truncate the hashes so that different columns collide
      const unsigned long long mask = strtoull(e, nullptr, 0);
      for (auto &v : hash) v &= mask;
    }
    // duplicated(mat, MARGIN = 2) among the non-constant columns: the first column of each hash class is kept; a later
    // member is removed once a bitwise comparison on the device has confirmed it (a 128-bit collision is not ruled out)
    struct Key { unsigned long long a, b; bool operator==(const Key &o) const { return a == o.a && b == o.b; } };
    struct KeyHash { size_t operator()(const Key &k) const { return (size_t)(k.a ^ (k.b * 0x9e3779b97f4a7c15ull)); } };
    std::unordered_map<Key, std::vector<int>, KeyHash> seen;   // hash -> kept columns with that hash (normally one)
    std::vector<int> pairs, cand;
    for (int j = 0; j < p; j++) {
      if (h->bool_cst[j]) continue;
      Key k{hash[2 * (size_t)j], hash[2 * (size_t)j + 1]};
      auto it = seen.find(k);
      if (it == seen.end()) { seen[k] = {j}; continue; }
      cand.push_back(j);
      pairs.push_back(it->second[0]);
      pairs.push_back(j);
    }
    if (!cand.empty()) {
      std::vector<int> out(cand.size(), 0);
      AQ_TRY(dpairs_.alloc(pairs.size()));
      AQ_TRY(dout_.alloc(out.size()));
      int *const dpairs = dpairs_.get(), *const dout = dout_.get();
      AQ_HIP(hipMemcpy(dpairs, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice));
      AQ_HIP(hipMemset(dout, 0, out.size() * sizeof(int)));
      hipLaunchKernelGGL((aq_k_cols_equal<T>), dim3((unsigned)cand.size()), dim3(256), 0, 0, dX, n, dmean, dsd, dpairs, dout);
      AQ_HIP(hipMemcpy(out.data(), dout, out.size() * sizeof(int), hipMemcpyDeviceToHost));
      // A candidate the bitwise comparison found DIFFERENT from the first column of its hash class (a 128-bit collision) is a
      // column of its own: it joins the class, and every later candidate of the class that differs from the first member is
      // compared with the further members as well, in column order (one pair per launch: this never happens in practice).
      auto equal_on_device = [&](int ca, int cb, bool *eq) -> int {
        const int pr2[2] = {ca, cb};
        int res = 0;
        if (hipMemcpy(dpairs, pr2, sizeof(pr2), hipMemcpyHostToDevice) != hipSuccess || hipMemset(dout, 0, sizeof(int)) != hipSuccess)
          return aq_fail(AQ_ERR_DEVICE, "aq_prepare_data: duplicate check failed");
        hipLaunchKernelGGL((aq_k_cols_equal<T>), dim3(1), dim3(256), 0, 0, dX, n, dmean, dsd, dpairs, dout);
        if (hipMemcpy(&res, dout, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
          return aq_fail(AQ_ERR_DEVICE, "aq_prepare_data: duplicate check failed");
        *eq = (res == 0);
        return AQ_OK;
      };
      for (size_t c = 0; c < cand.size(); c++) {
        const int j = cand[c];
        if (out[c] == 0) { h->bool_coll[j] = 1; h->dup_of[j] = pairs[2 * c]; continue; }
        std::vector<int> &members = seen[Key{hash[2 * (size_t)j], hash[2 * (size_t)j + 1]}];
        bool dup = false;
        for (size_t m = 1; m < members.size() && !dup; m++) {
          bool eq = false;
          AQ_TRY(equal_on_device(members[m], j, &eq));
          if (eq) { h->bool_coll[j] = 1; h->dup_of[j] = members[m]; dup = true; }
        }
        if (!dup) members.push_back(j);
      }
    }
    int kept = 0;
    for (int j = 0; j < p; j++)
      if (!h->bool_cst[j] && !h->bool_coll[j]) dst[j] = kept++;
    h->p_kept = kept;
    if (kept < 1) return aq_fail(AQ_ERR_ARG, "There must be at least 1 non-constant candidate predictor stored in X.");
    AQ_TRY(ddst.alloc((size_t)p));
    AQ_HIP(hipMemcpy(ddst.get(), dst.data(), (size_t)p * sizeof(int), hipMemcpyHostToDevice));
    AQ_TRY(h->Xs.alloc((size_t)n * kept));
    hipLaunchKernelGGL((aq_k_standardise<T>), dim3(p), dim3(256), 0, 0, dX, n, dmean, dsd, ddst.get(), h->Xs.get(), (unsigned long long *)nullptr);
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipDeviceSynchronize());
  }
  return AQ_OK;
}

// brings the host matrix to the device and runs the pipeline on it
template <typename T>
static int aq_prepare_x(aq_prep *h, const T *X_host) {
  const size_t np = (size_t)h->n * h->p;
  AqDev<T> dX;
  AQ_TRY(dX.alloc(np));
  AQ_HIP(hipMemcpy(dX.get(), X_host, np * sizeof(T), hipMemcpyHostToDevice));
  return aq_prepare_x_device<T>(h, dX.get());
}

// ---- covariates: the basis on the host, the two residual passes on the device ----
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
static int aq_cov_host_basis(const aq_prep_cov *cov, int n, const char *who, std::vector<double> *Q) {
  if (!cov->Z) return aq_fail(AQ_ERR_ARG, std::string(who) + ": NULL covariate pointer");
  AQ_TRY(aq_cov_check_dims(n, cov->d));
  Q->resize((size_t)n * (cov->d + 1));
  return aq_cov_basis(cov->Z, n, cov->d, Q->data(), nullptr);
}

// x_j <- x_j - Q (Q' x_j) for every column of the device matrix dX into dXr (dX itself for T = double)
template <typename T>
static int aq_cov_residualise_x(aq_prep *h, const T *dX, double *dXr, const double *dQt, int D) {
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

// host matrix -> device, residuals on the covariates as fp64, then the fp64 pipeline on them
template <typename T>
static int aq_prepare_x_cov(aq_prep *h, const T *X_host, const double *dQt, int D) {
  const size_t np = (size_t)h->n * h->p;
  AqDev<T> dX;
  AqDev<double> dXr;
  AQ_TRY(dX.alloc(np));
  AQ_HIP(hipMemcpy(dX.get(), X_host, np * sizeof(T), hipMemcpyHostToDevice));
  double *xr;
  if constexpr (std::is_same<T, double>::value) {
    xr = dX.get();
  } else {
    AQ_TRY(dXr.alloc(np));
    xr = dXr.get();
  }
  AQ_TRY(aq_cov_residualise_x<T>(h, dX.get(), xr, dQt, D));
  if constexpr (!std::is_same<T, double>::value) dX.reset();
  return aq_prepare_x_device<double>(h, xr);
}

extern "C" void aq_prep_destroy(aq_prep_handle h) {
  if (!h) return;
  hipSetDevice(h->device);
  delete h;
}

// the transform argument of aq_prepare_data_opt, before any device call (method 0 asks for nothing and is not looked at further)
static int aq_ytrans_check_args(const aq_prep_ytrans *yt, int n, const char *who) {
  if (yt->method == 0) return AQ_OK;
  if (yt->method != 1)
    return aq_fail(AQ_ERR_ARG, std::string(who) + ": unknown transform of Y, method = " + std::to_string(yt->method) +
                                   " (0 none, 1 rank-based inverse normal)");
  AQ_TRY(aq_ytrans_check_offset(yt->offset, who));
  if (n > AQ_N_MAX)
    return aq_fail(AQ_ERR_ARG, std::string(who) + ": n = " + std::to_string(n) + " exceeds the largest supported sample count, n <= " +
                                   std::to_string(AQ_N_MAX) + " (AQ_N_MAX)");
  return AQ_OK;
}

// Y <- scale(Y, center = TRUE, scale = FALSE) into h->Yc and the two missingness guards (R/prepare_atlasqtl.R:39-45, :83)
// With covariates (dQt: their basis [D][n] on the device) the residuals on [1, Z] over each column's observed rows take the
// place of the centring, and a column on whose observed rows the covariates are collinear is an error after the two guards.
// With a transform (yt, checked by the caller) the columns are rank-normalised in place on the device before either, and a
// column without two distinct observed values is an error after the two guards.
static int aq_prepare_y(aq_prep *h, const double *Y_host, const double *dQt = nullptr, int D = 0, const aq_prep_ytrans *yt = nullptr) {
  const int n = h->n, q = h->q;
  const size_t nq = (size_t)n * q;
  AqDev<double> dY;
  AqDev<int> dnobs, dflag;
  std::vector<int> nobs(q), flag;
  AQ_TRY(dY.alloc(nq));
  AQ_TRY(h->Yc.alloc(nq));
  AQ_TRY(dnobs.alloc((size_t)q));
  AQ_HIP(hipMemcpy(dY.get(), Y_host, nq * sizeof(double), hipMemcpyHostToDevice));
  std::vector<int> yt_deg;
  if (yt && yt->method != 0) {
    AqDev<int> dyo, dyt, dyd;
    AQ_TRY(dyo.alloc((size_t)q));
    AQ_TRY(dyt.alloc((size_t)q));
    AQ_TRY(dyd.alloc((size_t)q));
    AQ_TRY(aq_ytrans_device(dY.get(), dY.get(), n, q, yt->offset, dyo.get(), dyt.get(), dyd.get(), "aq_prepare_data_opt", nullptr));
    h->yt_method = yt->method;
    h->yt_offset = yt->offset;
    h->yt_nobs.resize(q); h->yt_ntied.resize(q); yt_deg.resize(q);
    AQ_HIP(hipMemcpy(h->yt_nobs.data(), dyo.get(), (size_t)q * sizeof(int), hipMemcpyDeviceToHost));
    AQ_HIP(hipMemcpy(h->yt_ntied.data(), dyt.get(), (size_t)q * sizeof(int), hipMemcpyDeviceToHost));
    AQ_HIP(hipMemcpy(yt_deg.data(), dyd.get(), (size_t)q * sizeof(int), hipMemcpyDeviceToHost));
  }
  if (dQt) {
    AQ_TRY(dflag.alloc_zeroed((size_t)q));
    hipLaunchKernelGGL(aq_k_cov_residualise_y, dim3(q), dim3(256), aq_cov_y_lds_bytes(D), 0, dY.get(), n, D, dQt, h->Yc.get(), dnobs.get(),
                       dflag.get());
    AQ_HIP(hipGetLastError());
    flag.resize(q);
    AQ_HIP(hipMemcpy(flag.data(), dflag.get(), flag.size() * sizeof(int), hipMemcpyDeviceToHost));
  } else {
    hipLaunchKernelGGL(aq_k_centre_y, dim3(q), dim3(256), 0, 0, dY.get(), n, h->Yc.get(), dnobs.get());
    AQ_HIP(hipGetLastError());
  }
  AQ_HIP(hipMemcpy(nobs.data(), dnobs.get(), nobs.size() * sizeof(int), hipMemcpyDeviceToHost));
  {
    long long tot = 0;
    std::string low;
    for (int k = 0; k < q; k++) {
      tot += nobs[k];
      if ((double)nobs[k] / n < 0.025) low += (low.empty() ? "" : " ") + std::to_string(k + 1);
    }
    if ((double)tot / ((double)n * q) < 0.05) return aq_fail(AQ_ERR_ARG, "Too few non-NA values in matrix Y. Exit.");
    if (!low.empty())
      return aq_fail(AQ_ERR_ARG, "Column(s) " + low + " of matrix Y have more than 97.5% missing values, and should be removed. Exit.");
  }
  if (!yt_deg.empty()) AQ_TRY(aq_ytrans_check_degenerate(yt_deg.data(), q));
  for (size_t k = 0; k < flag.size(); k++)
    if (flag[k])
      return aq_fail(AQ_ERR_ARG, "covariates are collinear on the samples observed for column " + std::to_string(k + 1) + " of Y (" +
                                     std::to_string(nobs[k]) + " observed, " + std::to_string(D - 1) + " covariates and the intercept)");
  return AQ_OK;
}

// cov == NULL or cov->d == 0: no covariates, the path of aq_prepare_data
static int aq_prepare_data_impl(const aq_prep_input *in, const aq_prep_cov *cov, aq_prep_handle *out, const std::string &who,
                                const aq_prep_ytrans *yt = nullptr) {
  if (!in || !out) return aq_fail(AQ_ERR_ARG, who + ": NULL argument");
  *out = nullptr;
  if (in->n < 2 || in->p < 1 || in->q < 1) return aq_fail(AQ_ERR_ARG, who + ": n >= 2, p >= 1, q >= 1 required");
  if ((!in->X && !in->X_i8) || !in->Y) return aq_fail(AQ_ERR_ARG, who + ": NULL data pointer");
  if (yt) AQ_TRY(aq_ytrans_check_args(yt, in->n, who.c_str()));
  const bool with_cov = cov && cov->d != 0;
  std::vector<double> Q;
  if (with_cov) AQ_TRY(aq_cov_host_basis(cov, in->n, who.c_str(), &Q));
  AQ_TRY(aq_need_device(in->device));
  const size_t np = (size_t)in->n * in->p;
  if (in->X)
    for (size_t i = 0; i < np; i++)   // check_structure_(X, "matrix", "numeric"): no NA, finite (R/utils.R:34-100)
      if (!std::isfinite(in->X[i])) return aq_fail(AQ_ERR_ARG, "X must be a non-empty a numeric matrix, finite without missing value.");
  std::unique_ptr<aq_prep> h(new aq_prep());
  h->n = in->n; h->p = in->p; h->q = in->q; h->device = in->device;
  if (with_cov) {
    const int D = cov->d + 1;
    AqDev<double> dQt;   // n x D column-major = [D][n]
    AQ_TRY(dQt.alloc(Q.size()));
    AQ_HIP(hipMemcpy(dQt.get(), Q.data(), Q.size() * sizeof(double), hipMemcpyHostToDevice));
    AQ_TRY(in->X ? aq_prepare_x_cov<double>(h.get(), in->X, dQt.get(), D) : aq_prepare_x_cov<int8_t>(h.get(), in->X_i8, dQt.get(), D));
    AQ_TRY(aq_prepare_y(h.get(), in->Y, dQt.get(), D, yt));
  } else {
    AQ_TRY(in->X ? aq_prepare_x<double>(h.get(), in->X) : aq_prepare_x<int8_t>(h.get(), in->X_i8));
    AQ_TRY(aq_prepare_y(h.get(), in->Y, nullptr, 0, yt));
  }
  *out = h.release();
  return AQ_OK;
}

extern "C" int aq_prepare_data(const aq_prep_input *in, aq_prep_handle *out) {
  return aq_prepare_data_impl(in, nullptr, out, "aq_prepare_data");
}

extern "C" int aq_prepare_data_cov(const aq_prep_input *in, const aq_prep_cov *cov, aq_prep_handle *out) {
  return aq_prepare_data_impl(in, cov, out, cov && cov->d != 0 ? "aq_prepare_data_cov" : "aq_prepare_data");
}

// ---- PLINK 1 .bed input: 2 bits per genotype, unpacked on the device (include/atlasqtl_hip.h, aq_prepare_data_bed) ----
#define AQ_BED_NA (-128)   // a missing genotype in the int8 dosage buffer (never a dosage)

// four 2-bit codes (one .bed byte) -> four dosage bytes, the missing code (1) -> AQ_BED_NA
__device__ __forceinline__ uint32_t aq_bed_dosage4(uint32_t b, int count_a2) {
  uint32_t x = b & 0xffu;
  x = (x | (x << 12)) & 0x000f000fu;
  x = (x | (x << 6)) & 0x03030303u;            // code s in byte s
  const uint32_t H = (x >> 1) & 0x01010101u, L = x & 0x01010101u;
  const uint32_t M = L & ~H;                   // missing
  uint32_t d = H + (H & L);                    // A2 dosage: 0 (hom A1), 1 (het), 2 (hom A2)
  if (!count_a2) d = 0x02020202u - d;          // A1 dosage (every byte <= 2: no borrow between bytes)
  return (d & ~(M * 0xffu)) | (M << 7);
}

__device__ __forceinline__ int8_t aq_bed_dosage1(uint32_t code, int count_a2) {
  if (code == 1) return (int8_t)AQ_BED_NA;
  const int a2 = (int)(code >> 1) + (int)(code == 3);
  return (int8_t)(count_a2 ? a2 : 2 - a2);
}

__device__ __forceinline__ int aq_wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Decode without sample selection: one wave per variant, four variants per workgroup.  The dosage column j starts at byte
// j n of G, its packed block at byte j stride of bed: neither is aligned in general.  The column is cut where its OUTPUT is
// 16-byte aligned: a lane takes 16 genotypes = 32 bits of the block, at any bit offset, out of two aligned dwords (the
// buffer is padded so that both exist) and writes one aligned 16-byte vector; the up to 15 genotypes before the first and
// after the last full vector go one per lane.  The four codes are counted on the packed words (popcount), summed over the
// wave and written by one lane.  All offsets are 64-bit.
__global__ __launch_bounds__(256) void aq_k_bed_decode(const uint32_t *__restrict__ bed32, long long stride, int n, int p,
                                                      int count_a2, int8_t *__restrict__ G, int32_t *__restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= p) return;
  const uint8_t *bed8 = (const uint8_t *)bed32;
  const long long out0 = j * (long long)n, in0 = j * stride;
  const int lead = (int)min((long long)n, (16 - (out0 & 15)) & 15);
  const int nvec = (n - lead) >> 4;
  const int tail0 = lead + (nvec << 4);
  int c_het = 0, c_hom2 = 0, c_mis = 0;
  for (int k = lane; k < nvec; k += 64) {
    const int s0 = lead + (k << 4);
    const long long bit = (in0 << 3) + ((long long)s0 << 1);
    const long long di = bit >> 5;
    const int sh = (int)(bit & 31);
    const unsigned long long ww = ((unsigned long long)bed32[di + 1] << 32) | bed32[di];
    const uint32_t w = (uint32_t)(ww >> sh);
    const uint32_t lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
    c_mis += __popc(lo & ~hi);
    c_het += __popc(hi & ~lo);
    c_hom2 += __popc(hi & lo);
    uint4 v;
    v.x = aq_bed_dosage4(w, count_a2);
    v.y = aq_bed_dosage4(w >> 8, count_a2);
    v.z = aq_bed_dosage4(w >> 16, count_a2);
    v.w = aq_bed_dosage4(w >> 24, count_a2);
    *reinterpret_cast<uint4 *>(G + out0 + s0) = v;
  }
  const int nsingle = lead + (n - tail0);       // <= 30
  if (lane < nsingle) {
    const int s = lane < lead ? lane : tail0 + (lane - lead);
    const uint32_t code = (bed8[in0 + (s >> 2)] >> (2 * (s & 3))) & 3u;
    c_mis += (code == 1); c_het += (code == 2); c_hom2 += (code == 3);
    G[out0 + s] = aq_bed_dosage1(code, count_a2);
  }
  c_mis = aq_wave_sum(c_mis); c_het = aq_wave_sum(c_het); c_hom2 = aq_wave_sum(c_hom2);
  if (lane == 0) {
    int32_t *c = counts + 4 * j;
    c[0] = n - c_mis - c_het - c_hom2; c[1] = c_het; c[2] = c_hom2; c[3] = c_mis;
  }
}

// Decode with sample selection: row i of the column is file sample idx[i], gathered bytewise out of the variant's block
__global__ __launch_bounds__(256) void aq_k_bed_gather(const uint8_t *__restrict__ bed8, long long stride, int n, int p,
                                                      const int32_t *__restrict__ idx, int count_a2, int8_t *__restrict__ G,
                                                      int32_t *__restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= p) return;
  const long long out0 = j * (long long)n, in0 = j * stride;
  int c_het = 0, c_hom2 = 0, c_mis = 0;
  for (int i = lane; i < n; i += 64) {
    const int s = idx[i];
    const uint32_t code = (bed8[in0 + (s >> 2)] >> (2 * (s & 3))) & 3u;
    c_mis += (code == 1); c_het += (code == 2); c_hom2 += (code == 3);
    G[out0 + i] = aq_bed_dosage1(code, count_a2);
  }
  c_mis = aq_wave_sum(c_mis); c_het = aq_wave_sum(c_het); c_hom2 = aq_wave_sum(c_hom2);
  if (lane == 0) {
    int32_t *c = counts + 4 * j;
    c[0] = n - c_mis - c_het - c_hom2; c[1] = c_het; c[2] = c_hom2; c[3] = c_mis;
  }
}

// int8 dosages -> fp64 with the variant's own value (fill[j]) in place of a missing genotype
__global__ __launch_bounds__(256) void aq_k_bed_impute(const int8_t *__restrict__ G, int n, const double *__restrict__ fill,
                                                      double *__restrict__ X) {
  const size_t base = (size_t)blockIdx.x * n;
  const double f = fill[blockIdx.x];
  for (int i = threadIdx.x; i < n; i += 256) {
    const int8_t g = G[base + i];
    X[base + i] = g == (int8_t)AQ_BED_NA ? f : (double)g;
  }
}

// the decode pass: packed blocks -> *dG_out (n x p int8, AQ_BED_NA = missing) and h->gcounts
static int aq_bed_decode(aq_prep *h, const aq_prep_bed_input *in, AqDev<int8_t> *dG_out) {
  const int n = h->n, p = h->p;
  const size_t stride = ((size_t)in->n_file + 3) / 4, nbytes = (size_t)p * stride;
  AqDev<uint32_t> dbed;
  AqDev<int32_t> didx, dcnt;
  const unsigned grid = (unsigned)(((long long)p + 3) / 4);
  // two dwords of padding: the aligned pair a lane reads may end one dword past the last block (those bits are shifted out)
  AQ_TRY(dbed.alloc(nbytes / 4 + 3));
  AQ_HIP(hipMemcpy(dbed.get(), in->bed, nbytes, hipMemcpyHostToDevice));
  AQ_TRY(dG_out->alloc((size_t)n * p));
  AQ_TRY(dcnt.alloc((size_t)4 * p));
  if (in->sample_idx) {
    AQ_TRY(didx.alloc((size_t)n));
    AQ_HIP(hipMemcpy(didx.get(), in->sample_idx, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(aq_k_bed_gather, dim3(grid), dim3(256), 0, 0, (const uint8_t *)dbed.get(), (long long)stride, n, p, didx.get(),
                       in->count_a2, dG_out->get(), dcnt.get());
  } else {
    hipLaunchKernelGGL(aq_k_bed_decode, dim3(grid), dim3(256), 0, 0, dbed.get(), (long long)stride, n, p, in->count_a2, dG_out->get(), dcnt.get());
  }
  AQ_HIP(hipGetLastError());
  h->gcounts.resize((size_t)4 * p);
  AQ_HIP(hipMemcpy(h->gcounts.data(), dcnt.get(), h->gcounts.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  return AQ_OK;
}

static int aq_prepare_data_bed_impl(const aq_prep_bed_input *in, const aq_prep_cov *cov, aq_prep_handle *out,
                                    const aq_prep_ytrans *yt = nullptr) {
  if (!in || !out) return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: NULL argument");
  *out = nullptr;
  if (in->n < 2 || in->p < 1 || in->q < 1) return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: n >= 2, p >= 1, q >= 1 required");
  if (!in->bed || !in->Y) return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: NULL data pointer");
  if (in->n > in->n_file)
    return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: n = " + std::to_string(in->n) + " rows asked of a file with n_file = " +
                                       std::to_string(in->n_file) + " samples");
  if (!in->sample_idx && in->n != in->n_file)
    return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: sample_idx is NULL, so n = " + std::to_string(in->n) +
                                       " must equal n_file = " + std::to_string(in->n_file));
  if (in->sample_idx)
    for (int i = 0; i < in->n; i++)
      if (in->sample_idx[i] < 0 || in->sample_idx[i] >= in->n_file)
        return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: sample_idx[" + std::to_string(i) + "] = " +
                                           std::to_string(in->sample_idx[i]) + " is out of range [0, " + std::to_string(in->n_file) + ")");
  if ((in->count_a2 != 0 && in->count_a2 != 1) || (in->missing != 0 && in->missing != 1))
    return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: count_a2 and missing must be 0 or 1");
  if (yt) AQ_TRY(aq_ytrans_check_args(yt, in->n, "aq_prepare_data_bed"));
  const bool with_cov = cov && cov->d != 0;
  const int D = with_cov ? cov->d + 1 : 0;
  std::vector<double> Q;
  if (with_cov) AQ_TRY(aq_cov_host_basis(cov, in->n, "aq_prepare_data_bed_cov", &Q));
  AQ_TRY(aq_need_device(in->device));
  std::unique_ptr<aq_prep> h(new aq_prep());
  h->n = in->n; h->p = in->p; h->q = in->q; h->device = in->device;
  AqDev<int8_t> dG;
  AqDev<double> dX, dfill, dQt;
  long long n_mis = 0, p_mis = 0, first_mis = -1;
  if (with_cov) {
    AQ_TRY(dQt.alloc(Q.size()));
    AQ_HIP(hipMemcpy(dQt.get(), Q.data(), Q.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  AQ_TRY(aq_bed_decode(h.get(), in, &dG));
  for (int j = 0; j < in->p; j++) {
    const int m = h->gcounts[4 * (size_t)j + 3];
    if (m > 0) { n_mis += m; p_mis++; if (first_mis < 0) first_mis = j; }
  }
  if (n_mis == 0 && with_cov) {   // the decoded dosages enter the residual pass as int8; its fp64 output enters the pipeline
    AQ_TRY(dX.alloc((size_t)in->n * in->p));
    AQ_TRY(aq_cov_residualise_x<int8_t>(h.get(), dG.get(), dX.get(), dQt.get(), D));
    dG.reset();
    AQ_TRY(aq_prepare_x_device<double>(h.get(), dX.get()));
  } else if (n_mis == 0) {
    AQ_TRY(aq_prepare_x_device<int8_t>(h.get(), dG.get()));
  } else if (!in->missing) {
    return aq_fail(AQ_ERR_ARG, "X must be a non-empty a numeric matrix, finite without missing value. " + std::to_string(n_mis) +
                                     " genotype(s) in " + std::to_string(p_mis) + " variant(s) are missing among the " +
                                     std::to_string(in->n) + " samples used; the first such variant has index " +
                                     std::to_string(first_mis) + " (0-based, among the variants given). missing = \"mean\" replaces "
                                     "a missing genotype by the mean of its variant's observed ones.");
  } else {
    std::vector<double> fill(in->p);
    for (int j = 0; j < in->p; j++) {   // (n_het + 2 n_hom_counted) / n_obs: one fp64 division of exact integers
      const int32_t *c = &h->gcounts[4 * (size_t)j];
      const int n_obs = c[0] + c[1] + c[2];
      fill[j] = n_obs > 0 ? (double)(c[1] + 2 * (long long)(in->count_a2 ? c[2] : c[0])) / (double)n_obs : 0.0;
    }
    AQ_TRY(dfill.alloc((size_t)in->p));
    AQ_HIP(hipMemcpy(dfill.get(), fill.data(), (size_t)in->p * sizeof(double), hipMemcpyHostToDevice));
    AQ_TRY(dX.alloc((size_t)in->n * in->p));
    hipLaunchKernelGGL(aq_k_bed_impute, dim3(in->p), dim3(256), 0, 0, dG.get(), in->n, dfill.get(), dX.get());
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipDeviceSynchronize());
    dG.reset();
    if (with_cov) AQ_TRY(aq_cov_residualise_x<double>(h.get(), dX.get(), dX.get(), dQt.get(), D));   // in place
    AQ_TRY(aq_prepare_x_device<double>(h.get(), dX.get()));
  }
  dG.reset();
  dX.reset();
  AQ_TRY(with_cov ? aq_prepare_y(h.get(), in->Y, dQt.get(), D, yt) : aq_prepare_y(h.get(), in->Y, nullptr, 0, yt));
  *out = h.release();
  return AQ_OK;
}

extern "C" int aq_prepare_data_bed(const aq_prep_bed_input *in, aq_prep_handle *out) { return aq_prepare_data_bed_impl(in, nullptr, out); }

extern "C" int aq_prepare_data_bed_cov(const aq_prep_bed_input *in, const aq_prep_cov *cov, aq_prep_handle *out) {
  return aq_prepare_data_bed_impl(in, cov, out);
}

extern "C" int aq_prep_cov_info(aq_prep_handle h, int32_t *d, uint8_t *absorbed, double *r2) {
  if (!h) return aq_fail(AQ_ERR_ARG, "NULL handle");
  if (d) *d = h->n_cov;
  if (absorbed) std::copy(h->cov_absorbed.begin(), h->cov_absorbed.end(), absorbed);
  if (r2) std::copy(h->cov_r2.begin(), h->cov_r2.end(), r2);
  return AQ_OK;
}

// ---- the four entries in one, with the transform of Y (include/atlasqtl_hip.h, aq_prepare_data_opt; kernels in aq_ytrans_kernels.h) ----
extern "C" int aq_prepare_data_opt(const aq_prep_input *in, const aq_prep_bed_input *bed, const aq_prep_cov *cov, const aq_prep_ytrans *yt,
                                   aq_prep_handle *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_prepare_data_opt: NULL argument");
  *out = nullptr;
  if ((in == nullptr) == (bed == nullptr)) return aq_fail(AQ_ERR_ARG, "aq_prepare_data_opt: exactly one of in and bed must be non-NULL");
  const bool with_cov = cov && cov->d != 0;
  if (!yt || yt->method == 0) {                // exactly the entry that the other arguments name
    if (in) return aq_prepare_data_impl(in, cov, out, with_cov ? "aq_prepare_data_cov" : "aq_prepare_data");
    return aq_prepare_data_bed_impl(bed, cov, out);
  }
  if (in) return aq_prepare_data_impl(in, cov, out, "aq_prepare_data_opt", yt);
  return aq_prepare_data_bed_impl(bed, cov, out, yt);
}

extern "C" int aq_prep_ytrans_info(aq_prep_handle h, int32_t *method, double *offset, int32_t *n_obs, int32_t *n_tied) {
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_ytrans_info: NULL handle");
  if (method) *method = h->yt_method;
  if (h->yt_method == 0) return AQ_OK;
  if (offset) *offset = h->yt_offset;
  if (n_obs) std::copy(h->yt_nobs.begin(), h->yt_nobs.end(), n_obs);
  if (n_tied) std::copy(h->yt_ntied.begin(), h->yt_ntied.end(), n_tied);
  return AQ_OK;
}

extern "C" int aq_rank_int(const double *Y, int32_t n, int32_t q, double offset, double *out, int32_t *n_obs, int32_t *n_tied, int32_t device) {
  if (!Y || !out) return aq_fail(AQ_ERR_ARG, "aq_rank_int: NULL argument");
  if (n < 2 || q < 1) return aq_fail(AQ_ERR_ARG, "aq_rank_int: n >= 2, q >= 1 required");
  const aq_prep_ytrans yt{1, offset};
  AQ_TRY(aq_ytrans_check_args(&yt, n, "aq_rank_int"));
  AQ_TRY(aq_need_device(device));
  const size_t nq = (size_t)n * q;
  AqDev<double> dY;
  AqDev<int> dcnt;                             // n_obs, n_tied, degenerate: q each
  std::vector<int> cnt((size_t)3 * q);
  AQ_TRY(dY.alloc(nq));
  AQ_TRY(dcnt.alloc(cnt.size()));
  AQ_HIP(hipMemcpy(dY.get(), Y, nq * sizeof(double), hipMemcpyHostToDevice));
  AQ_TRY(aq_ytrans_device(dY.get(), dY.get(), n, q, offset, dcnt.get(), dcnt.get() + q, dcnt.get() + 2 * (size_t)q, "aq_rank_int", nullptr));
  AQ_HIP(hipMemcpy(cnt.data(), dcnt.get(), cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
  AQ_TRY(aq_ytrans_check_degenerate(cnt.data() + 2 * (size_t)q, q));
  AQ_HIP(hipMemcpy(out, dY.get(), nq * sizeof(double), hipMemcpyDeviceToHost));
  if (n_obs) std::copy(cnt.begin(), cnt.begin() + q, n_obs);
  if (n_tied) std::copy(cnt.begin() + q, cnt.begin() + 2 * (size_t)q, n_tied);
  return AQ_OK;
}

extern "C" int aq_ytrans_plan_query(int32_t n, int32_t q, int64_t free_bytes, aq_ytrans_plan *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_ytrans_plan_query: NULL argument");
  *out = aq_ytrans_plan{};
  std::string err;
  const int rc = aq_ytrans_make_plan(n, q, (long long)free_bytes, aq_ytrans_env_force(), "aq_ytrans_plan_query", out, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

// ---- LD pruning of a finished handle (include/atlasqtl_hip.h, aq_prep_ld_prune; kernels in aq_ld_kernels.h) ----
static int aq_ld_check_window(int32_t window, const char *who) {
  if (window < 1 || window > AQ_LD_MAX_WINDOW)
    return aq_fail(AQ_ERR_ARG, std::string(who) + ": window must lie in [1, " + std::to_string(AQ_LD_MAX_WINDOW) + "], " +
                                   std::to_string(window) + " given");
  return AQ_OK;
}

// the f64 MFMA accumulator map the band kernel is written for (row = (lane >> 4) + 4 reg), checked on the device
static int aq_ld_need_layout(const char *who) {
  int dmode = 0;
  AQ_TRY(aq_probe_dmode(&dmode));
  if (dmode != 0)
    return aq_fail(AQ_ERR_DEVICE, std::string(who) + ": the band kernel is written for the accumulator map row = (lane >> 4) + 4 reg "
                                                     "of v_mfma_f64_16x16x4_f64, which this device does not have");
  return AQ_OK;
}

static dim3 aq_ld_grid(int p1, int window) { return dim3((unsigned)((p1 + 63) / 64), (unsigned)((window + 63) / 64)); }

extern "C" int aq_prep_ld_prune(aq_prep_handle h, const aq_prep_ld *ld) {
  if (!ld) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_prune: NULL argument");
  AQ_TRY(aq_ld_check_window(ld->window, "aq_prep_ld_prune"));
  if (!(ld->r2 > 0.0 && ld->r2 <= 1.0))
    return aq_fail(AQ_ERR_ARG, "aq_prep_ld_prune: r2 must lie in (0, 1], " + std::to_string(ld->r2) + " given");
  if (ld->window_bp > 0 && !ld->pos)
    return aq_fail(AQ_ERR_ARG, "aq_prep_ld_prune: window_bp = " + std::to_string(ld->window_bp) + " needs the positions (pos is NULL)");
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_prune: NULL handle");
  if (h->ld_done) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_prune: the handle has been pruned already (once per handle)");
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_ld_need_layout("aq_prep_ld_prune"));
  const int n = h->n, p = h->p, p1 = h->p_kept, window = ld->window, nw = (window + 63) / 64;
  const bool with_pos = ld->window_bp > 0;
  std::vector<int32_t> orig;                   // compact index -> original column
  orig.reserve((size_t)p1);
  for (int j = 0; j < p; j++)
    if (!h->bool_cst[j] && !h->bool_coll[j]) orig.push_back(j);
  AqDev<int32_t> dgroup, dof, ddst;
  AqDev<long long> dpos;
  AqDev<unsigned long long> dbits;
  AqDev<uint8_t> dbool;
  AqDev<double> dr2, Xnew;
  if (ld->group) {
    std::vector<int32_t> cg((size_t)p1);
    for (int c = 0; c < p1; c++) cg[c] = ld->group[orig[c]];
    AQ_TRY(dgroup.alloc((size_t)p1));
    AQ_HIP(hipMemcpy(dgroup.get(), cg.data(), cg.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  if (with_pos) {
    std::vector<long long> cp((size_t)p1);
    for (int c = 0; c < p1; c++) cp[c] = (long long)ld->pos[orig[c]];
    AQ_TRY(dpos.alloc((size_t)p1));
    AQ_HIP(hipMemcpy(dpos.get(), cp.data(), cp.size() * sizeof(long long), hipMemcpyHostToDevice));
  }
  AQ_TRY(dbits.alloc((size_t)p1 * nw));
  AQ_TRY(dbool.alloc((size_t)p1));
  AQ_TRY(dof.alloc((size_t)p1));
  AQ_TRY(dr2.alloc((size_t)p1));
  hipLaunchKernelGGL((aq_k_ld_band<true>), aq_ld_grid(p1, window), dim3(256), 0, 0, h->Xs.get(), n, p1, window, ld->r2, dgroup.get(),
                     dpos.get(), with_pos ? (long long)ld->window_bp : 0ll, (double *)nullptr, dbits.get(), nw);
  hipLaunchKernelGGL(aq_k_ld_scan, dim3(1), dim3(64), 0, 0, dbits.get(), p1, nw, dbool.get(), dof.get());
  hipLaunchKernelGGL(aq_k_ld_tag_r2, dim3(p1), dim3(256), 0, 0, h->Xs.get(), n, dof.get(), dr2.get());
  AQ_HIP(hipGetLastError());
  std::vector<uint8_t> rm((size_t)p1);
  std::vector<int32_t> of((size_t)p1), dst((size_t)p1, -1);
  std::vector<double> r2((size_t)p1);
  AQ_HIP(hipMemcpy(rm.data(), dbool.get(), rm.size(), hipMemcpyDeviceToHost));
  AQ_HIP(hipMemcpy(of.data(), dof.get(), of.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  AQ_HIP(hipMemcpy(r2.data(), dr2.get(), r2.size() * sizeof(double), hipMemcpyDeviceToHost));
  int p2 = 0;
  for (int c = 0; c < p1; c++)
    if (!rm[c]) dst[c] = p2++;
  if (p2 < p1) {                               // gather the kept columns, then release the matrix they came from
    AQ_TRY(ddst.alloc((size_t)p1));
    AQ_HIP(hipMemcpy(ddst.get(), dst.data(), dst.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    AQ_TRY(Xnew.alloc((size_t)n * p2));
    hipLaunchKernelGGL(aq_k_ld_gather, dim3(p1), dim3(256), 0, 0, h->Xs.get(), n, ddst.get(), Xnew.get());
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipDeviceSynchronize());
    h->Xs = std::move(Xnew);
  }
  h->ld_removed.assign((size_t)p, 0);
  h->ld_of.assign((size_t)p, -1);
  h->ld_r2.assign((size_t)p, std::nan(""));
  for (int c = 0; c < p1; c++)
    if (rm[c]) {
      h->ld_removed[orig[c]] = 1;
      h->ld_of[orig[c]] = orig[of[c]];
      h->ld_r2[orig[c]] = r2[c];
    }
  h->p_kept = p2;
  h->ld_done = true;
  return AQ_OK;
}

extern "C" int aq_prep_ld_info(aq_prep_handle h, int32_t *p_kept, uint8_t *bool_ld, int32_t *ld_of, double *ld_r2) {
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_info: NULL handle");
  if (!h->ld_done) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_info: aq_prep_ld_prune has not run on the handle");
  if (p_kept) *p_kept = h->p_kept;
  if (bool_ld) std::copy(h->ld_removed.begin(), h->ld_removed.end(), bool_ld);
  if (ld_of) std::copy(h->ld_of.begin(), h->ld_of.end(), ld_of);
  if (ld_r2) std::copy(h->ld_r2.begin(), h->ld_r2.end(), ld_r2);
  return AQ_OK;
}

extern "C" int aq_prep_ld_band(aq_prep_handle h, int32_t window, double *r_band) {
  AQ_TRY(aq_ld_check_window(window, "aq_prep_ld_band"));
  if (!h || !r_band) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_band: NULL argument");
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_ld_need_layout("aq_prep_ld_band"));
  const int p1 = h->p_kept;
  const size_t len = (size_t)p1 * window;
  AqDev<double> dband;
  AQ_TRY(dband.alloc(len));
  hipLaunchKernelGGL((aq_k_ld_band<false>), aq_ld_grid(p1, window), dim3(256), 0, 0, h->Xs.get(), h->n, p1, window, 1.0,
                     (const int32_t *)nullptr, (const long long *)nullptr, 0ll, dband.get(), (unsigned long long *)nullptr, 0);
  AQ_HIP(hipGetLastError());
  AQ_HIP(hipMemcpy(r_band, dband.get(), len * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}

// ---- the genetic relationship matrix of a finished handle (include/atlasqtl_hip.h, aq_prep_grm; kernels in aq_grm_kernels.h) ----
extern "C" int aq_grm_plan_query(int32_t n, int32_t p1, int32_t ncu, int64_t free_bytes, aq_grm_plan *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_grm_plan_query: NULL argument");
  *out = aq_grm_plan{};
  std::string err;
  const int rc = aq_grm_make_plan(n, p1, ncu, (long long)free_bytes, 0, "aq_grm_plan_query", out, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

template <int T, bool A16>
static void aq_grm_launch_partial(const aq_grm_plan &pl, const double *Xs, int n, int p1, double *scratch) {
  hipLaunchKernelGGL((aq_k_grm_partial<T, A16>), dim3((unsigned)pl.n_tiles, (unsigned)pl.splits), dim3(256), 0, 0, Xs, n, p1, pl.splits,
                     pl.chunks_per_split, scratch);
}

// the two kernels on the handle's current matrix: K (n x n) in dK, the partial tiles in scratch.  Asynchronous.
static int aq_grm_launch(aq_prep *h, const aq_grm_plan &pl, double *scratch, double *dK) {
  const bool a16 = (h->n & 1) == 0;            // even n: every column starts at a multiple of 16 bytes
  auto launch = pl.tile == 128 ? (a16 ? aq_grm_launch_partial<128, true> : aq_grm_launch_partial<128, false>)
                               : (a16 ? aq_grm_launch_partial<64, true> : aq_grm_launch_partial<64, false>);
  launch(pl, h->Xs.get(), h->n, h->p_kept, scratch);
  const int nb = pl.tile / 16;
  hipLaunchKernelGGL(aq_k_grm_reduce, dim3((unsigned)pl.n_tiles, (unsigned)(nb * nb)), dim3(256), 0, 0, scratch, pl.tile, h->n, h->p_kept,
                     pl.splits, dK);
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

// the plan of a handle on its device: CU count and free memory from the runtime, AQ_GRM_SPLITS from the environment
static int aq_grm_plan_for(aq_prep *h, const char *who, aq_grm_plan *pl) {
  hipDeviceProp_t prop;
  size_t free_b = 0, tot_b = 0;
  AQ_HIP(hipGetDeviceProperties(&prop, h->device));
  AQ_HIP(hipMemGetInfo(&free_b, &tot_b));
  int force = 0;
  if (const char *e = getenv("AQ_GRM_SPLITS")) {   // test hook: that many splits whatever p1 is
    force = atoi(e);
    if (force < 1) return aq_fail(AQ_ERR_ARG, std::string(who) + ": AQ_GRM_SPLITS must lie in [1, " + std::to_string(AQ_GRM_MAX_SPLITS) + "]");
  }
  std::string err;
  const int rc = aq_grm_make_plan(h->n, h->p_kept, prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256, (long long)free_b, force,
                                  who, pl, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

extern "C" int aq_prep_grm(aq_prep_handle h, double *K_out, double *trace_out) {
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_grm: NULL handle");
  if (!K_out) return aq_fail(AQ_ERR_ARG, "aq_prep_grm: NULL output");
  std::string err;
  if (aq_grm_check_n(h->n, "aq_prep_grm", &err) != AQ_OK) return aq_fail(AQ_ERR_UNSUPPORTED, err);
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_ld_need_layout("aq_prep_grm"));
  const size_t n = (size_t)h->n;
  aq_grm_plan pl{};
  AQ_TRY(aq_grm_plan_for(h, "aq_prep_grm", &pl));
  AqDev<double> dK, scratch;
  AQ_TRY(dK.alloc(n * n));
  AQ_TRY(scratch.alloc((size_t)pl.scratch_bytes / sizeof(double)));
  AQ_TRY(aq_grm_launch(h, pl, scratch.get(), dK.get()));
  AQ_HIP(hipMemcpy(K_out, dK.get(), n * n * sizeof(double), hipMemcpyDeviceToHost));
  if (trace_out) {                             // the diagonal as returned, added in index order
    double tr = 0.0;
    for (size_t i = 0; i < n; i++) tr += K_out[i * n + i];
    *trace_out = tr;
  }
  return AQ_OK;
}

// Timing hook of aq_prep_grm: the two kernels alone, `reps` times between two events, without the copy to the host.
extern "C" int aq_prep_grm_time(aq_prep_handle h, int32_t reps, double *ms_per_call, aq_grm_plan *plan_out) {
  if (!h || !ms_per_call) return aq_fail(AQ_ERR_ARG, "aq_prep_grm_time: NULL argument");
  if (reps < 1) return aq_fail(AQ_ERR_ARG, "aq_prep_grm_time: reps >= 1 required");
  std::string err;
  if (aq_grm_check_n(h->n, "aq_prep_grm_time", &err) != AQ_OK) return aq_fail(AQ_ERR_UNSUPPORTED, err);
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_ld_need_layout("aq_prep_grm_time"));
  aq_grm_plan pl{};
  AQ_TRY(aq_grm_plan_for(h, "aq_prep_grm_time", &pl));
  if (plan_out) *plan_out = pl;
  AqDev<double> dK, scratch;
  AQ_TRY(dK.alloc((size_t)h->n * h->n));
  AQ_TRY(scratch.alloc((size_t)pl.scratch_bytes / sizeof(double)));
  AQ_TRY(aq_grm_launch(h, pl, scratch.get(), dK.get()));   // warm-up
  AQ_HIP(hipDeviceSynchronize());
  struct Events {                              // both destroyed on every way out
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() {
      for (hipEvent_t ev : e)
        if (ev) hipEventDestroy(ev);
    }
  } ev;
  AQ_HIP(hipEventCreate(&ev.e[0]));
  AQ_HIP(hipEventCreate(&ev.e[1]));
  AQ_HIP(hipEventRecord(ev.e[0], 0));
  for (int r = 0; r < reps; r++) AQ_TRY(aq_grm_launch(h, pl, scratch.get(), dK.get()));
  AQ_HIP(hipEventRecord(ev.e[1], 0));
  AQ_HIP(hipEventSynchronize(ev.e[1]));
  float ms = 0.f;
  AQ_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  *ms_per_call = (double)ms / reps;
  return AQ_OK;
}

// ---- the relationship operator applied to a block of vectors (include/atlasqtl_hip.h, aq_prep_grm_apply; kernels in aq_pcs_kernels.h) ----
extern "C" int aq_pcs_plan_query(int32_t n, int32_t p1, int32_t L, int32_t ncu, int64_t free_bytes, aq_pcs_plan *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_pcs_plan_query: NULL argument");
  *out = aq_pcs_plan{};
  std::string err;
  const int rc = aq_pcs_make_plan(n, p1, L, ncu, (long long)free_bytes, 0, "aq_pcs_plan_query", out, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

static int aq_pcs_check_l(int32_t L, const char *who) {
  if (L < 1 || L > AQ_PCS_MAX_L)
    return aq_fail(AQ_ERR_ARG, std::string(who) + ": L must lie in [1, " + std::to_string(AQ_PCS_MAX_L) + "], " + std::to_string(L) + " given");
  return AQ_OK;
}

// the plan of a handle on its device: CU count and free memory from the runtime, AQ_PCS_SPLITS from the environment
static int aq_pcs_plan_for(aq_prep *h, int L, const char *who, aq_pcs_plan *pl) {
  hipDeviceProp_t prop;
  size_t free_b = 0, tot_b = 0;
  AQ_HIP(hipGetDeviceProperties(&prop, h->device));
  AQ_HIP(hipMemGetInfo(&free_b, &tot_b));
  int force = 0;
  if (const char *e = getenv("AQ_PCS_SPLITS")) {   // test hook: that many splits of the second product whatever p1 is
    force = atoi(e);
    if (force < 1) return aq_fail(AQ_ERR_ARG, std::string(who) + ": AQ_PCS_SPLITS must lie in [1, " + std::to_string(AQ_PCS_MAX_SPLITS) + "]");
  }
  std::string err;
  const int rc = aq_pcs_make_plan(h->n, h->p_kept, L, prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256, (long long)free_b,
                                  force, who, pl, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

// the device buffers of one application: Q and Z as the caller has them, Q packed, T and the partial tiles
struct AqPcsBuf {
  AqDev<double> Q, Qt, T, scratch, Z;
  int alloc(const aq_pcs_plan &pl, int n, int L) {
    AQ_TRY(Q.alloc((size_t)n * L));
    AQ_TRY(Z.alloc((size_t)n * L));
    AQ_TRY(Qt.alloc((size_t)pl.n_pad * pl.lp));
    AQ_TRY(T.alloc((size_t)pl.t_bytes / sizeof(double)));
    AQ_TRY(scratch.alloc((size_t)pl.scratch_bytes / sizeof(double)));
    return AQ_OK;
  }
};

template <int NL, bool A16>
static void aq_pcs_launch_products(const aq_pcs_plan &pl, const double *Xs, int n, int p1, AqPcsBuf &b) {
  hipLaunchKernelGGL((aq_k_pcs_xtq<NL, A16>), dim3((unsigned)pl.n_panels), dim3(256), 0, 0, Xs, n, p1, pl.n_pad, b.Qt.get(), b.T.get());
  hipLaunchKernelGGL((aq_k_pcs_xt<NL, A16>), dim3((unsigned)pl.n_tiles, (unsigned)pl.splits), dim3(256), 0, 0, Xs, n, p1, pl.splits,
                     pl.chunks_per_split, b.T.get(), b.scratch.get());
}

template <bool A16>
static void aq_pcs_launch_width(int nl, const aq_pcs_plan &pl, const double *Xs, int n, int p1, AqPcsBuf &b) {
  switch (nl) {                                // one instance per padded width lp = 16 nl
    case 1: return aq_pcs_launch_products<1, A16>(pl, Xs, n, p1, b);
    case 2: return aq_pcs_launch_products<2, A16>(pl, Xs, n, p1, b);
    case 3: return aq_pcs_launch_products<3, A16>(pl, Xs, n, p1, b);
    case 4: return aq_pcs_launch_products<4, A16>(pl, Xs, n, p1, b);
    case 5: return aq_pcs_launch_products<5, A16>(pl, Xs, n, p1, b);
    case 6: return aq_pcs_launch_products<6, A16>(pl, Xs, n, p1, b);
    case 7: return aq_pcs_launch_products<7, A16>(pl, Xs, n, p1, b);
    default: return aq_pcs_launch_products<8, A16>(pl, Xs, n, p1, b);
  }
}

// the four kernels on the handle's current matrix: b.Q (n x L) -> b.Z (n x L).  Asynchronous.
static int aq_pcs_launch(aq_prep *h, const aq_pcs_plan &pl, int L, AqPcsBuf &b) {
  const int n = h->n, p1 = h->p_kept, nl = pl.lp / 16;
  const long long cells = (long long)pl.n_pad * pl.lp;
  hipLaunchKernelGGL(aq_k_pcs_pack_q, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, 0, b.Q.get(), n, L, pl.n_pad, pl.lp, b.Qt.get());
  if ((n & 1) == 0)                            // even n: every column starts at a multiple of 16 bytes
    aq_pcs_launch_width<true>(nl, pl, h->Xs.get(), n, p1, b);
  else
    aq_pcs_launch_width<false>(nl, pl, h->Xs.get(), n, p1, b);
  hipLaunchKernelGGL(aq_k_pcs_reduce, dim3((unsigned)pl.n_tiles, (unsigned)((L + 3) / 4)), dim3(256), 0, 0, b.scratch.get(), n, p1, L, pl.lp,
                     pl.splits, b.Z.get());
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

extern "C" int aq_prep_grm_apply(aq_prep_handle h, const double *Q, int32_t L, double *Z_out, double *trace_out) {
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_grm_apply: NULL handle");
  if (!Q || !Z_out) return aq_fail(AQ_ERR_ARG, "aq_prep_grm_apply: NULL argument");
  AQ_TRY(aq_pcs_check_l(L, "aq_prep_grm_apply"));
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_ld_need_layout("aq_prep_grm_apply"));
  const size_t n = (size_t)h->n, p1 = (size_t)h->p_kept;
  aq_pcs_plan pl{};
  AQ_TRY(aq_pcs_plan_for(h, L, "aq_prep_grm_apply", &pl));
  AqPcsBuf b;
  AQ_TRY(b.alloc(pl, h->n, L));
  AQ_HIP(hipMemcpy(b.Q.get(), Q, n * L * sizeof(double), hipMemcpyHostToDevice));
  AQ_TRY(aq_pcs_launch(h, pl, L, b));
  AQ_HIP(hipMemcpy(Z_out, b.Z.get(), n * L * sizeof(double), hipMemcpyDeviceToHost));
  if (trace_out) {                             // the columns' sums of squares, added in index order
    AqDev<double> dss;
    AQ_TRY(dss.alloc(p1));
    hipLaunchKernelGGL(aq_k_pcs_colss, dim3((unsigned)p1), dim3(256), 0, 0, h->Xs.get(), h->n, dss.get());
    AQ_HIP(hipGetLastError());
    std::vector<double> ss(p1);
    AQ_HIP(hipMemcpy(ss.data(), dss.get(), p1 * sizeof(double), hipMemcpyDeviceToHost));
    double tr = 0.0;
    for (size_t j = 0; j < p1; j++) tr += ss[j];
    *trace_out = tr / (double)p1;
  }
  return AQ_OK;
}

// Timing hook of aq_prep_grm_apply: the four kernels alone on a block of ones, `reps` times between two events, without the
// copies from and to the host.
extern "C" int aq_prep_grm_apply_time(aq_prep_handle h, int32_t L, int32_t reps, double *ms_per_call, aq_pcs_plan *plan_out) {
  if (!h || !ms_per_call) return aq_fail(AQ_ERR_ARG, "aq_prep_grm_apply_time: NULL argument");
  if (reps < 1) return aq_fail(AQ_ERR_ARG, "aq_prep_grm_apply_time: reps >= 1 required");
  AQ_TRY(aq_pcs_check_l(L, "aq_prep_grm_apply_time"));
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_ld_need_layout("aq_prep_grm_apply_time"));
  aq_pcs_plan pl{};
  AQ_TRY(aq_pcs_plan_for(h, L, "aq_prep_grm_apply_time", &pl));
  if (plan_out) *plan_out = pl;
  AqPcsBuf b;
  AQ_TRY(b.alloc(pl, h->n, L));
  {
    std::vector<double> ones((size_t)h->n * L, 1.0);
    AQ_HIP(hipMemcpy(b.Q.get(), ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  AQ_TRY(aq_pcs_launch(h, pl, L, b));          // warm-up
  AQ_HIP(hipDeviceSynchronize());
  struct Events {                              // both destroyed on every way out
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() {
      for (hipEvent_t ev : e)
        if (ev) hipEventDestroy(ev);
    }
  } ev;
  AQ_HIP(hipEventCreate(&ev.e[0]));
  AQ_HIP(hipEventCreate(&ev.e[1]));
  AQ_HIP(hipEventRecord(ev.e[0], 0));
  for (int r = 0; r < reps; r++) AQ_TRY(aq_pcs_launch(h, pl, L, b));
  AQ_HIP(hipEventRecord(ev.e[1], 0));
  AQ_HIP(hipEventSynchronize(ev.e[1]));
  float ms = 0.f;
  AQ_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  *ms_per_call = (double)ms / reps;
  return AQ_OK;
}

extern "C" int aq_prep_genotype_counts(aq_prep_handle h, int32_t *counts) {
  if (!h || !counts) return aq_fail(AQ_ERR_ARG, "aq_prep_genotype_counts: NULL argument");
  if (h->gcounts.empty())
    return aq_fail(AQ_ERR_ARG, "aq_prep_genotype_counts: the handle was not made by aq_prepare_data_bed");
  std::copy(h->gcounts.begin(), h->gcounts.end(), counts);
  return AQ_OK;
}

extern "C" int aq_prep_info(aq_prep_handle h, int32_t *p_kept, uint8_t *bool_cst, uint8_t *bool_coll, int32_t *dup_of,
                            double *x_mean, double *x_sd) {
  if (!h) return aq_fail(AQ_ERR_ARG, "NULL handle");
  if (p_kept) *p_kept = h->p_kept;
  if (bool_cst) std::copy(h->bool_cst.begin(), h->bool_cst.end(), bool_cst);
  if (bool_coll) std::copy(h->bool_coll.begin(), h->bool_coll.end(), bool_coll);
  if (dup_of) std::copy(h->dup_of.begin(), h->dup_of.end(), dup_of);
  if (x_mean) std::copy(h->mean.begin(), h->mean.end(), x_mean);
  if (x_sd) std::copy(h->sd.begin(), h->sd.end(), x_sd);
  return AQ_OK;
}

extern "C" const double *aq_prep_x_device(aq_prep_handle h) { return h ? h->Xs.get() : nullptr; }
extern "C" const double *aq_prep_y_device(aq_prep_handle h) { return h ? h->Yc.get() : nullptr; }

extern "C" int aq_prep_get(aq_prep_handle h, double *X_out, double *Y_out) {
  if (!h) return aq_fail(AQ_ERR_ARG, "NULL handle");
  if (hipSetDevice(h->device) != hipSuccess) return aq_fail(AQ_ERR_DEVICE, "hipSetDevice failed");
  if (X_out && hipMemcpy(X_out, h->Xs.get(), (size_t)h->n * h->p_kept * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return aq_fail(AQ_ERR_DEVICE, "aq_prep_get: copy of X failed");
  if (Y_out && hipMemcpy(Y_out, h->Yc.get(), (size_t)h->n * h->q * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return aq_fail(AQ_ERR_DEVICE, "aq_prep_get: copy of Y failed");
  return AQ_OK;
}
