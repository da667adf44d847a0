// aq_prep_cis.hip -- the cis scan of a finished prepare handle (include/atlasqtl_hip.h): aq_prep_cis tests every trait against
// the predictors of its own window on the f64 matrix pipe (aq_cis_kernels.h; order, work items and plan by aq_cis_plan.h) and
// returns the selected pairs, each trait's best in-window predictor and its undefined pairs; aq_prep_cis_perm evaluates the
// same statistic on permuted responses and returns each trait's largest in-window r^2 per permutation; aq_prep_cis_time times
// the kernels alone, aq_cis_plan_query runs the planner on the host.  The kernels are plain HIP that issues no hand-written
// load: the ISA proof of the look-ahead sweep units does not cover them and need not.
#include "aq_cis_host.h"      // AqCisBuf, aq_cis_setup, aq_cis_*_args, aq_cis_colstats, aq_cis_launch_scan, aq_cis_launch_tile,
                              // aq_cis_upload_time_cut, aq_cis_copy_scan, aq_cis_need_windows; aq_screen_host.h, aq_prep.h,
                              // aq_cis_kernels.h
#include "aq_msperm_plan.h"   // aq_msperm_check_rows (the plan header alone: aq_msperm_kernels.h defines a non-static kernel)

extern "C" int aq_cis_plan_query(int32_t n, int32_t p1, int32_t q, int32_t masked, int32_t ncu, const int32_t *s_lo, const int32_t *s_hi,
                                 int32_t n_perm, aq_cis_plan *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_cis_plan_query: NULL argument");
  *out = aq_cis_plan{};
  std::string err;
  const int rc = aq_cis_make_plan(n, p1, q, masked, ncu, s_lo, s_hi, n_perm, 0, 0, "aq_cis_plan_query", out, nullptr, &err);
  if (rc != AQ_OK) *out = aq_cis_plan{};
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

// every kernel of one scan after aq_cis_setup: the launch sequence of aq_cis_host.h around the gather of the ordered copy of
// Y and the plain tile kernel.  Asynchronous.
static int aq_cis_launch_plain(aq_prep *h, AqCisBuf &b) {
  return aq_cis_launch_scan(h, b, true, [&](unsigned W, const aq_cis_args &a) {
    const int qa = b.wk.q_active;
    hipLaunchKernelGGL(aq_k_ms_gather, dim3((unsigned)(qa < (1 << 20) ? qa : (1 << 20))), dim3(256), 0, 0, h->Yc.get(),
                       (const int32_t *)b.order.get(), (const int32_t *)nullptr, h->n, qa, 1, b.Yo.get());
    if (b.pl.masked)
      aq_cis_launch_tile<true>(W, a);
    else
      aq_cis_launch_tile<false>(W, a);
  });
}

template <bool MASKED, int PB>
static void aq_cis_launch_perm_tile(unsigned grid, const aq_cis_args &a) {
  aq_screen_a16(a.n, [&](auto a16) {
    hipLaunchKernelGGL((aq_k_cis_perm_tile<MASKED, decltype(a16)::value, PB>), dim3(grid), dim3(256), 0, 0, a);
  });
}

// the kernels of one launch over the nb <= batch permutations whose rows lie in b.perm; Sx and Sxx have been formed.
// Asynchronous.
static int aq_cis_launch_perm(aq_prep *h, AqCisBuf &b, int nb) {
  const int q = h->q, qa = b.wk.q_active, pb = b.pl.pb;
  const long long W = b.pl.n_items;
  AQ_HIP(hipMemsetAsync(b.key.get(), 0, (size_t)nb * (size_t)q * sizeof(unsigned long long), 0));
  if (W > 0) {
    const long long cols = (long long)nb * (long long)qa;
    hipLaunchKernelGGL(aq_k_ms_gather, dim3((unsigned)(cols < (1ll << 20) ? cols : (1ll << 20))), dim3(256), 0, 0, h->Yc.get(),
                       (const int32_t *)b.order.get(), (const int32_t *)b.perm.get(), h->n, qa, nb, b.Yp.get());
    aq_cis_args a = aq_cis_common_args(h, b);
    a.Yo = b.Yp.get();
    a.nb = nb;
    a.key = b.key.get();
    const unsigned grid = (unsigned)(W * ((nb + pb - 1) / pb));   // < 2^31: the plan
    if (b.pl.masked) {
      if (pb == 2)
        aq_cis_launch_perm_tile<true, 2>(grid, a);
      else
        aq_cis_launch_perm_tile<true, 1>(grid, a);
    } else if (pb == 4) {
      aq_cis_launch_perm_tile<false, 4>(grid, a);
    } else if (pb == 2) {
      aq_cis_launch_perm_tile<false, 2>(grid, a);
    } else {
      aq_cis_launch_perm_tile<false, 1>(grid, a);
    }
  }
  const long long count = (long long)nb * (long long)q;
  hipLaunchKernelGGL(aq_k_cis_reduce, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, b.key.get(), count, b.max_r2.get());
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}


extern "C" int aq_prep_cis(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const double *r2_cut, int64_t cap, int32_t *snp,
                           int32_t *trait, double *r, int64_t *n_pairs, int32_t *best_snp, double *best_r, int64_t *n_undef,
                           aq_cis_plan *plan_out) {
  if (!s_lo || !s_hi || !r2_cut) return aq_fail(AQ_ERR_ARG, "aq_prep_cis: NULL s_lo, s_hi or r2_cut");
  if (cap < 0) return aq_fail(AQ_ERR_ARG, "aq_prep_cis: cap >= 0 required, " + std::to_string(cap) + " given");
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_cis: NULL handle");
  AQ_TRY(aq_cis_need_windows(h, s_lo, s_hi, "aq_prep_cis"));
  AQ_TRY(aq_screen_need_cut(r2_cut, h->q, "aq_prep_cis"));
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_cis"));
  AqCisBuf b;
  AQ_TRY(aq_cis_setup(h, s_lo, s_hi, r2_cut, cap, true, 0, "aq_prep_cis", &b));
  if (plan_out) *plan_out = b.pl;
  AQ_TRY(aq_cis_launch_plain(h, b));
  return aq_cis_copy_scan(h, b, snp, trait, r, n_pairs, best_snp, best_r, n_undef);
}

extern "C" int aq_prep_cis_perm(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, int32_t n_perm, const int32_t *perm,
                                double *max_r2) {
  if (n_perm < 1) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_perm: n_perm >= 1 required, " + std::to_string(n_perm) + " given");
  if (!s_lo || !s_hi || !perm) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_perm: NULL s_lo, s_hi or perm");
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_perm: NULL handle");
  AQ_TRY(aq_cis_need_windows(h, s_lo, s_hi, "aq_prep_cis_perm"));
  {
    std::string err;                             // an index out of range never reaches the gather kernel
    const int rc = aq_msperm_check_rows(perm, n_perm, h->n, "aq_prep_cis_perm", &err);
    if (rc != AQ_OK) return aq_fail(rc, err);
  }
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_cis_perm"));
  const size_t q = (size_t)h->q, n = (size_t)h->n;
  AqCisBuf b;
  AQ_TRY(aq_cis_setup(h, s_lo, s_hi, nullptr, 0, false, n_perm, "aq_prep_cis_perm", &b));
  AQ_TRY(aq_cis_colstats(h, b));
  for (int done = 0; done < n_perm; done += b.pl.batch) {
    const int nb = n_perm - done < b.pl.batch ? n_perm - done : b.pl.batch;
    AQ_HIP(hipMemcpy(b.perm.get(), perm + (size_t)done * n, (size_t)nb * n * sizeof(int32_t), hipMemcpyHostToDevice));
    AQ_TRY(aq_cis_launch_perm(h, b, nb));
    if (max_r2) AQ_HIP(hipMemcpy(max_r2 + (size_t)done * q, b.max_r2.get(), (size_t)nb * q * sizeof(double), hipMemcpyDeviceToHost));
    AQ_HIP(hipDeviceSynchronize());              // the next launch overwrites the buffers
  }
  return AQ_OK;
}

// Timing hook: the scan's kernels `reps` times between two events, counting only (cap = 0), with the cutoff of
// aq_prep_marginal_time (aq_screen_time_cut); then, with n_perm >= 1, the gather, tile and reduce kernels of n_perm
// permutations launch by launch, on one batch of the rows of aq_prep_marginal_perm_time (aq_screen_time_perms).
extern "C" int aq_prep_cis_time(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, int32_t n_perm, int32_t reps, double *ms_scan,
                                double *ms_per_perm, aq_cis_plan *plan_out) {
  if (!s_lo || !s_hi || !ms_scan || !ms_per_perm) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_time: NULL argument");
  if (n_perm < 0 || reps < 1) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_time: n_perm >= 0 and reps >= 1 required");
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_time: NULL handle");
  AQ_TRY(aq_cis_need_windows(h, s_lo, s_hi, "aq_prep_cis_time"));
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_cis_time"));
  const size_t n = (size_t)h->n;
  AqCisBuf b;
  AQ_TRY(aq_cis_setup(h, s_lo, s_hi, nullptr, 0, true, n_perm, "aq_prep_cis_time", &b));
  if (plan_out) *plan_out = b.pl;
  AQ_TRY(aq_cis_upload_time_cut(b, [&](size_t j) { return b.mt_host[j] - 2 - h->n_cov; }));
  AQ_TRY(aq_time_launches(reps, ms_scan, [&] { return aq_cis_launch_plain(h, b); }));
  *ms_per_perm = 0.0;
  if (n_perm > 0) {
    const std::vector<int32_t> perm = aq_screen_time_perms((size_t)b.pl.batch, n);
    AQ_HIP(hipMemcpy(b.perm.get(), perm.data(), perm.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    double ms = 0.0;
    AQ_TRY(aq_time_launches(reps, &ms, [&] {
      for (int done = 0; done < n_perm; done += b.pl.batch)
        AQ_TRY(aq_cis_launch_perm(h, b, n_perm - done < b.pl.batch ? n_perm - done : b.pl.batch));
      return (int)AQ_OK;
    }));
    *ms_per_perm = ms / (double)n_perm;
  }
  return AQ_OK;
}
