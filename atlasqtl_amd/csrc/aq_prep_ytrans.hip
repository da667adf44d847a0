// aq_prep_ytrans.hip -- the rank-based inverse normal transform of the traits (include/atlasqtl_hip.h; kernels in
// aq_ytrans_kernels.h, planned by aq_ytrans_plan.h): the check of the transform argument, the sequencing of the two kernels on a
// device-resident Y, which aq_prepare_y of aq_prepare.hip puts in front of everything else that is done to Y, and the entries of
// the transform alone: aq_rank_int, aq_ytrans_plan_query, aq_prep_ytrans_info.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>
#include "aq_prep.h"             // aq_prep, the prototypes of what aq_prepare.hip calls here; aq_internal.h
#include "aq_ytrans_kernels.h"   // aq_k_yt_lds, aq_k_yt_global; aq_ytrans_make_plan

// AQ_YT_PATH of the environment: 0 (absent), AQ_YT_FORCE_LDS, AQ_YT_FORCE_GLOBAL, or -1 for anything else
static int aq_ytrans_env_force() {
  const char *e = getenv("AQ_YT_PATH");
  if (!e || !*e) return 0;
  if (!strcmp(e, "lds")) return AQ_YT_FORCE_LDS;
  if (!strcmp(e, "global")) return AQ_YT_FORCE_GLOBAL;
  return -1;
}

// the transform argument of aq_prepare_data_opt, before any device call (method 0 asks for nothing and is not looked at further)
int aq_ytrans_check_args(const aq_prep_ytrans *yt, int n, const char *who) {
  if (yt->method == 0) return AQ_OK;
  if (yt->method != 1)
    return aq_fail(AQ_ERR_ARG, std::string(who) + ": unknown transform of Y, method = " + std::to_string(yt->method) +
                                   " (0 none, 1 rank-based inverse normal)");
  if (!(yt->offset >= 0.0 && yt->offset <= 0.5))   // NaN fails both
    return aq_fail(AQ_ERR_ARG, std::string(who) + ": the offset c must lie in [0, 1/2], " + std::to_string(yt->offset) + " given");
  if (n > AQ_N_MAX)
    return aq_fail(AQ_ERR_ARG, std::string(who) + ": n = " + std::to_string(n) + " exceeds the largest supported sample count, n <= " +
                                   std::to_string(AQ_N_MAX) + " (AQ_N_MAX)");
  return AQ_OK;
}

// dY (n x q column-major, device) -> dOut (may be dY); dnobs, dntied, ddeg: q ints each on the device.  Asynchronous after
// the plan: the caller's next copy from the device waits for the kernels.  The current device is the arrays' one.
int aq_ytrans_device(const double *dY, double *dOut, int n, int q, double c, int *dnobs, int *dntied, int *ddeg, const char *who,
                     aq_ytrans_plan *plan_out) {
  size_t free_b = 0, tot_b = 0;
  AQ_HIP(hipMemGetInfo(&free_b, &tot_b));
  aq_ytrans_plan pl{};
  std::string err;
  const int rc = aq_ytrans_make_plan(n, q, (long long)(free_b - free_b / 16), aq_ytrans_env_force(), who, &pl, &err);
  if (rc != AQ_OK) return aq_fail(rc, err);
  if (plan_out) *plan_out = pl;
  if (pl.path == 0) {
    const int half = pl.n_pad / 2;
    const int block = half < 64 ? 64 : (half > AQ_YT_BLOCK ? AQ_YT_BLOCK : half);
    AQ_HIP(hipFuncSetAttribute((const void *)aq_k_yt_lds, hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds_bytes));
    hipLaunchKernelGGL(aq_k_yt_lds, dim3((unsigned)q), dim3((unsigned)block), (size_t)pl.lds_bytes, 0, dY, n, pl.n_pad, c, dOut, dnobs, dntied, ddeg);
    AQ_HIP(hipGetLastError());
    return AQ_OK;
  }
  AqDev<uint64_t> keys;
  AQ_TRY(keys.alloc((size_t)pl.scratch_bytes / sizeof(uint64_t)));
  const int chunk = pl.lds_bytes / (int)sizeof(uint64_t);
  AQ_HIP(hipFuncSetAttribute((const void *)aq_k_yt_global, hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds_bytes));
  for (int k0 = 0; k0 < q; k0 += pl.traits_per_batch) {
    const int nb = q - k0 < pl.traits_per_batch ? q - k0 : pl.traits_per_batch;
    hipLaunchKernelGGL(aq_k_yt_global, dim3((unsigned)nb), dim3(AQ_YT_BLOCK), (size_t)pl.lds_bytes, 0, dY + (size_t)k0 * n, n, pl.n_pad, chunk, c,
                       dOut + (size_t)k0 * n, keys.get(), dnobs + k0, dntied + k0, ddeg + k0);
    AQ_HIP(hipGetLastError());
  }
  AQ_HIP(hipDeviceSynchronize());              // the scratch is released on return
  return AQ_OK;
}

// the first column that cannot be rank-normalised, if any
int aq_ytrans_check_degenerate(const int *deg, int q) {
  for (int k = 0; k < q; k++)
    if (deg[k])
      return aq_fail(AQ_ERR_ARG, "column " + std::to_string(k + 1) + " of Y has fewer than two distinct observed values; it cannot be "
                                     "rank-normalised");
  return AQ_OK;
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
