// aq_prep_grm.hip -- the genetic relationship matrix of a finished prepare handle and its application to a block of vectors
// (include/atlasqtl_hip.h).  aq_prep_grm forms K = Xs Xs' / p1 of the handle's current matrix on the f64 matrix pipe
// (aq_grm_kernels.h, planned by aq_grm_plan.h) and copies it to the host; aq_prep_grm_apply applies it without forming it,
// Xs (Xs' Q) / p1 (aq_pcs_kernels.h, planned by aq_pcs_plan.h): the step of subspace iteration for its leading eigenvectors, for
// any n a handle holds.  The two *_time entries time the kernels alone, the two *_plan_query entries run the planners on the
// host.  The kernels, two f64 MFMA families among them, are plain HIP that issues no hand-written load: the ISA proof of the
// look-ahead sweep units does not cover them and need not.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdint.h>
#include <string>
#include <vector>
#include "aq_prep.h"          // aq_prep, aq_time_launches; aq_internal.h: aq_fail, AQ_HIP, aq_need_device, aq_need_acc_layout, AqDev
#include "aq_grm_kernels.h"   // aq_k_grm_partial, aq_k_grm_reduce; aq_grm_make_plan
#include "aq_pcs_kernels.h"   // aq_k_pcs_pack_q, aq_k_pcs_xtq, aq_k_pcs_xt, aq_k_pcs_reduce, aq_k_pcs_colss; aq_pcs_make_plan

// what a planner takes from the handle's device and the environment: CU count and free memory from the runtime, and the
// number of splits that the variable `env` (AQ_GRM_SPLITS, AQ_PCS_SPLITS: test hooks) forces whatever p1 is (0: none)
struct AqPlanFacts { int ncu = 0, force = 0; long long free_bytes = 0; };
static int aq_plan_facts(const aq_prep *h, const char *env, int max_splits, const char *who, AqPlanFacts *f) {
  hipDeviceProp_t prop;
  size_t free_b = 0, tot_b = 0;
  AQ_HIP(hipGetDeviceProperties(&prop, h->device));
  AQ_HIP(hipMemGetInfo(&free_b, &tot_b));
  if (const char *e = getenv(env)) {
    f->force = atoi(e);
    if (f->force < 1) return aq_fail(AQ_ERR_ARG, std::string(who) + ": " + env + " must lie in [1, " + std::to_string(max_splits) + "]");
  }
  f->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  f->free_bytes = (long long)free_b;
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

// the plan of a handle on its device
static int aq_grm_plan_for(aq_prep *h, const char *who, aq_grm_plan *pl) {
  AqPlanFacts f;
  AQ_TRY(aq_plan_facts(h, "AQ_GRM_SPLITS", AQ_GRM_MAX_SPLITS, who, &f));
  std::string err;
  const int rc = aq_grm_make_plan(h->n, h->p_kept, f.ncu, f.free_bytes, f.force, who, pl, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

extern "C" int aq_prep_grm(aq_prep_handle h, double *K_out, double *trace_out) {
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_grm: NULL handle");
  if (!K_out) return aq_fail(AQ_ERR_ARG, "aq_prep_grm: NULL output");
  std::string err;
  if (aq_grm_check_n(h->n, "aq_prep_grm", &err) != AQ_OK) return aq_fail(AQ_ERR_UNSUPPORTED, err);
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_grm"));
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
  AQ_TRY(aq_need_acc_layout("aq_prep_grm_time"));
  aq_grm_plan pl{};
  AQ_TRY(aq_grm_plan_for(h, "aq_prep_grm_time", &pl));
  if (plan_out) *plan_out = pl;
  AqDev<double> dK, scratch;
  AQ_TRY(dK.alloc((size_t)h->n * h->n));
  AQ_TRY(scratch.alloc((size_t)pl.scratch_bytes / sizeof(double)));
  return aq_time_launches(reps, ms_per_call, [&] { return aq_grm_launch(h, pl, scratch.get(), dK.get()); });
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

// the plan of a handle on its device
static int aq_pcs_plan_for(aq_prep *h, int L, const char *who, aq_pcs_plan *pl) {
  AqPlanFacts f;
  AQ_TRY(aq_plan_facts(h, "AQ_PCS_SPLITS", AQ_PCS_MAX_SPLITS, who, &f));
  std::string err;
  const int rc = aq_pcs_make_plan(h->n, h->p_kept, L, f.ncu, f.free_bytes, f.force, who, pl, &err);
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
  AQ_TRY(aq_need_acc_layout("aq_prep_grm_apply"));
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
  AQ_TRY(aq_need_acc_layout("aq_prep_grm_apply_time"));
  aq_pcs_plan pl{};
  AQ_TRY(aq_pcs_plan_for(h, L, "aq_prep_grm_apply_time", &pl));
  if (plan_out) *plan_out = pl;
  AqPcsBuf b;
  AQ_TRY(b.alloc(pl, h->n, L));
  {
    std::vector<double> ones((size_t)h->n * L, 1.0);
    AQ_HIP(hipMemcpy(b.Q.get(), ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  return aq_time_launches(reps, ms_per_call, [&] { return aq_pcs_launch(h, pl, L, b); });
}
