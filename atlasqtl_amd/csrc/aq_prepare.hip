// aq_prepare.hip -- the O(n p) input construction of prepare_data_ on the device:
//   X <- scale(X)                                  R/prepare_atlasqtl.R:57   (centre, divide by the n - 1 standard deviation)
//   rm_constant_   (0/0 = NaN columns)             R/utils.R:276-302
//   rm_collinear_  (duplicated(mat, MARGIN = 2))   R/utils.R:304-343        (later copies of an identical column go)
//   Y <- scale(Y, center = TRUE, scale = FALSE)    R/prepare_atlasqtl.R:83   (column means over the observed entries)
//   and the two missingness guards                 R/prepare_atlasqtl.R:39-45
// and the one pipeline behind the five aq_prepare_data* entries (aq_prepare_run): a source step leaves the n x p matrix on the
// device -- an upload of fp64 values or of int8 dosages (0 / 1 / 2 ...: 1 byte per genotype, "block-standardised genotype X" of
// BASELINE.json configs[4]: at C5 that is 1 GB over PCIe instead of 8 GB, and the fp64 matrix never exists on the host), or the
// decode of a PLINK .bed (aq_prep_bed.hip) -- and one tail takes it from there: the residuals on the covariates, if any
// (aq_prep_cov.hip: fp64 on the device, freed once the compact matrix is written), the pipeline above on X, then Y with the
// rank-based inverse normal transform in front, if asked for (aq_prep_ytrans.hip).  The result stays on the device (compact
// n x p_kept fp64 + centred Y) and is handed to aq_vb_create as device pointers; aq_prep_info, aq_prep_get, aq_prep_x_device,
// aq_prep_y_device and aq_prep_destroy are here too.  The entries on a finished handle have units of their own:
// aq_prep_ld.hip, aq_prep_grm.hip.
// All of it is HBM-bound streaming: one read of X for the column statistics, one read + one write for the standardised
// matrix with its column hashes, one gather pass for the compaction.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <memory>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>
#include "aq_prep.h"       // aq_prep, the prototypes of the other aq_prep*.hip units; aq_internal.h: aq_fail, AQ_HIP, AqDev
#include "aq_prep_dev.h"   // aq_xval, aq_block_sum

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

// Y <- scale(Y, center = TRUE, scale = FALSE) into h->Yc and the two missingness guards (R/prepare_atlasqtl.R:39-45, :83)
// With covariates (dQt: their basis [D][n] on the device) the residuals on [1, Z] over each column's observed rows take the
// place of the centring, and a column on whose observed rows the covariates are collinear is an error after the two guards.
// With a transform (yt, checked by the caller) the columns are rank-normalised in place on the device before either, and a
// column without two distinct observed values is an error after the two guards.
static int aq_prepare_y(aq_prep *h, const double *Y_host, const double *dQt, int D, const aq_prep_ytrans *yt) {
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
    AQ_TRY(aq_cov_residualise_y(h, dY.get(), dQt, D, dnobs.get(), dflag.get()));
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

// The one pipeline behind the five entries.  `bed` says which of the two inputs is the entry's own (the other is NULL); `who` is
// the name the dense checks report under (the .bed checks always say aq_prepare_data_bed, its covariate checks
// aq_prepare_data_bed_cov).  Every check, the covariate basis included, runs on the host before the first device call.
static int aq_prepare_run(bool bed, const aq_prep_input *in, const aq_prep_bed_input *bin, const aq_prep_cov *cov, const aq_prep_ytrans *yt,
                          aq_prep_handle *out, const std::string &who) {
  if ((bed ? !bin : !in) || !out) return aq_fail(AQ_ERR_ARG, who + ": NULL argument");
  *out = nullptr;
  const int n = bed ? bin->n : in->n, p = bed ? bin->p : in->p, q = bed ? bin->q : in->q, device = bed ? bin->device : in->device;
  const double *Y = bed ? bin->Y : in->Y;
  if (n < 2 || p < 1 || q < 1) return aq_fail(AQ_ERR_ARG, who + ": n >= 2, p >= 1, q >= 1 required");
  if ((bed ? !bin->bed : (!in->X && !in->X_i8)) || !Y) return aq_fail(AQ_ERR_ARG, who + ": NULL data pointer");
  if (bed) AQ_TRY(aq_bed_check_args(bin));
  if (yt) AQ_TRY(aq_ytrans_check_args(yt, n, who.c_str()));
  const bool with_cov = cov && cov->d != 0;
  const int D = with_cov ? cov->d + 1 : 0;
  std::vector<double> Q;
  if (with_cov) AQ_TRY(aq_cov_host_basis(cov, n, bed ? "aq_prepare_data_bed_cov" : who.c_str(), &Q));
  AQ_TRY(aq_need_device(device));
  const size_t np = (size_t)n * p;
  if (!bed && in->X)
    for (size_t i = 0; i < np; i++)   // check_structure_(X, "matrix", "numeric"): no NA, finite (R/utils.R:34-100)
      if (!std::isfinite(in->X[i])) return aq_fail(AQ_ERR_ARG, "X must be a non-empty a numeric matrix, finite without missing value.");
  std::unique_ptr<aq_prep> h(new aq_prep());
  h->n = n; h->p = p; h->q = q; h->device = device;
  AqDev<int8_t> dG;           // the matrix as its source leaves it: int8 dosages here ...
  AqDev<double> dX, dQt;      // ... or fp64 here; the covariate basis, n x D column-major = [D][n]
  if (with_cov) {
    AQ_TRY(dQt.alloc(Q.size()));
    AQ_HIP(hipMemcpy(dQt.get(), Q.data(), Q.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  // the source step
  if (bed) {
    AQ_TRY(aq_bed_source(h.get(), bin, &dG, &dX));
  } else if (in->X) {
    AQ_TRY(dX.alloc(np));
    AQ_HIP(hipMemcpy(dX.get(), in->X, np * sizeof(double), hipMemcpyHostToDevice));
  } else {
    AQ_TRY(dG.alloc(np));
    AQ_HIP(hipMemcpy(dG.get(), in->X_i8, np, hipMemcpyHostToDevice));
  }
  // the tail.  Residuals on the covariates: of int8 dosages into a fresh fp64 matrix, after which the dosages go; of fp64 in place
  if (with_cov) {
    if (dG.get()) AQ_TRY(dX.alloc(np));
    AQ_TRY(aq_cov_residualise_x(h.get(), dG.get(), dX.get(), dQt.get(), D));
    dG.reset();
  }
  AQ_TRY(dG.get() ? aq_prepare_x_device<int8_t>(h.get(), dG.get()) : aq_prepare_x_device<double>(h.get(), dX.get()));
  dG.reset();
  dX.reset();
  AQ_TRY(aq_prepare_y(h.get(), Y, dQt.get(), D, yt));
  *out = h.release();
  return AQ_OK;
}

static bool aq_has_cov(const aq_prep_cov *cov) { return cov && cov->d != 0; }

extern "C" int aq_prepare_data(const aq_prep_input *in, aq_prep_handle *out) {
  return aq_prepare_run(false, in, nullptr, nullptr, nullptr, out, "aq_prepare_data");
}

extern "C" int aq_prepare_data_cov(const aq_prep_input *in, const aq_prep_cov *cov, aq_prep_handle *out) {
  return aq_prepare_run(false, in, nullptr, cov, nullptr, out, aq_has_cov(cov) ? "aq_prepare_data_cov" : "aq_prepare_data");
}

extern "C" int aq_prepare_data_bed(const aq_prep_bed_input *in, aq_prep_handle *out) {
  return aq_prepare_run(true, nullptr, in, nullptr, nullptr, out, "aq_prepare_data_bed");
}

extern "C" int aq_prepare_data_bed_cov(const aq_prep_bed_input *in, const aq_prep_cov *cov, aq_prep_handle *out) {
  return aq_prepare_run(true, nullptr, in, cov, nullptr, out, "aq_prepare_data_bed");
}

// the four entries above in one, with the transform of Y: the dense checks report under the name of the entry that the
// arguments name (aq_prepare_data_opt itself with a transform)
extern "C" int aq_prepare_data_opt(const aq_prep_input *in, const aq_prep_bed_input *bed, const aq_prep_cov *cov, const aq_prep_ytrans *yt,
                                   aq_prep_handle *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_prepare_data_opt: NULL argument");
  *out = nullptr;
  if ((in == nullptr) == (bed == nullptr)) return aq_fail(AQ_ERR_ARG, "aq_prepare_data_opt: exactly one of in and bed must be non-NULL");
  const char *who = bed ? "aq_prepare_data_bed" : (yt && yt->method != 0) ? "aq_prepare_data_opt" : aq_has_cov(cov) ? "aq_prepare_data_cov" : "aq_prepare_data";
  return aq_prepare_run(bed != nullptr, in, bed, cov, yt, out, who);
}

extern "C" void aq_prep_destroy(aq_prep_handle h) {
  if (!h) return;
  hipSetDevice(h->device);
  delete h;
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

// Test hook: column `col` of the standardised compact X replaced by `values` (n doubles), so that a test can plant what the
// preparation never leaves behind, a column of zeros for example.
extern "C" int aq_prep_debug_set_column(aq_prep_handle h, int32_t col, const double *values) {
  if (!h || !values) return aq_fail(AQ_ERR_ARG, "aq_prep_debug_set_column: NULL argument");
  if (col < 0 || col >= h->p_kept) return aq_fail(AQ_ERR_ARG, "aq_prep_debug_set_column: col outside [0, p_kept)");
  AQ_HIP(hipSetDevice(h->device));
  AQ_HIP(hipMemcpy(h->Xs.get() + (size_t)col * (size_t)h->n, values, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice));
  return AQ_OK;
}
