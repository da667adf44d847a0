// aq_prep_cis_int.hip -- the interaction cis scan of a finished prepare handle (include/atlasqtl_hip.h): aq_prep_cis_int tests,
// for every trait and every predictor of its own window, whether the predictor's effect depends on a sample-level variable e
// (aq_cisint_kernels.h; plan by aq_cisint_plan.h on top of aq_cis_plan.h) and returns what aq_prep_cis returns, and int_tol;
// aq_prep_cis_int_time times the kernels alone, aq_cisint_plan_query runs the planner on the host.  The kernels are plain HIP
// that issues no hand-written load: the ISA proof of the look-ahead sweep units does not cover them and need not.
#include "aq_cis_host.h"          // AqCisBuf, aq_cis_setup_complete, aq_cis_keep_syy, aq_cis_launch_scan, aq_cis_upload_time_cut,
                                  // aq_cis_copy_scan, aq_cis_need_windows; aq_screen_host.h
#include "aq_cisint_kernels.h"    // aq_k_ci_traits, aq_k_ci_predstats, aq_k_ci_tile; aq_cisint_make_plan, aq_cisint_check_basis

extern "C" int aq_cisint_plan_query(int32_t n, int32_t p1, int32_t q, int32_t ncu, const int32_t *s_lo, const int32_t *s_hi, int32_t n_basis,
                                    aq_cisint_plan *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_cisint_plan_query: NULL argument");
  *out = aq_cisint_plan{};
  std::string err;
  const int rc = aq_cisint_make_plan(n, p1, q, ncu, s_lo, s_hi, n_basis, "aq_cisint_plan_query", out, nullptr, &err);
  if (rc != AQ_OK) *out = aq_cisint_plan{};
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

// what the interaction adds to the buffers of a scan
struct AqCiBuf {
  AqCisBuf b;
  AqDev<double> B, mpad, syy0, vg, cgv, vw, tol;
  AqDev<int32_t> pok;
  aq_cisint_plan pl{};
};

// the arguments every entry checks before any device call, after its own first ones, in the order of the header
static int aq_ci_check(aq_prep *h, const int32_t *s_lo, const int32_t *s_hi, const double *basis, int n_basis, const double *mult,
                       const char *who) {
  std::string err;
  int rc = aq_cisint_check_nb(n_basis, who, &err);
  if (rc == AQ_OK) rc = aq_cisint_check_basis(basis, n_basis, mult, h->n, who, &err);
  if (rc != AQ_OK) return aq_fail(rc, err);
  return aq_cis_need_windows(h, s_lo, s_hi, who);
}

// the complete-Y set-up of aq_cis_host.h, the plan, the basis and the multiplier
static int aq_ci_setup(aq_prep *h, const int32_t *s_lo, const int32_t *s_hi, const double *basis, int n_basis, const double *mult,
                       const double *r2_cut, int64_t cap, const char *who, AqCiBuf *cb) {
  AqCisBuf &b = cb->b;
  AQ_TRY(aq_cis_setup_complete(h, s_lo, s_hi, r2_cut, cap, who, "interaction", &b));
  std::string err;
  // the cis plan inside is the same pure function of the same arguments as b.pl, and its order and work list are b.wk
  const int rc = aq_cisint_make_plan(h->n, h->p_kept, h->q, b.ncu, s_lo, s_hi, n_basis, who, &cb->pl, nullptr, &err);
  if (rc != AQ_OK) return aq_fail(rc, err);
  const size_t n = (size_t)h->n, p1 = (size_t)h->p_kept, npad = (size_t)cb->pl.mult_pad;
  AQ_TRY(cb->B.alloc((size_t)n_basis * n));
  AQ_TRY(cb->mpad.alloc(npad));
  AQ_TRY(cb->vg.alloc(p1));
  AQ_TRY(cb->cgv.alloc(p1));
  AQ_TRY(cb->vw.alloc(p1));
  AQ_TRY(cb->tol.alloc(p1));
  AQ_TRY(cb->pok.alloc(p1));
  AQ_HIP(hipMemcpy(cb->B.get(), basis, (size_t)n_basis * n * sizeof(double), hipMemcpyHostToDevice));
  AQ_HIP(hipMemset(cb->mpad.get(), 0, npad * sizeof(double)));
  AQ_HIP(hipMemcpy(cb->mpad.get(), mult, n * sizeof(double), hipMemcpyHostToDevice));
  return aq_cis_keep_syy(b, &cb->syy0);     // the trait kernel overwrites b.syy with S'yy_t
}

// the per-predictor statistics and the residual traits.  Asynchronous.
static int aq_ci_launch_stats(aq_prep *h, AqCiBuf &cb) {
  AqCisBuf &b = cb.b;
  const int qa = b.wk.q_active, nb = cb.pl.n_basis;
  hipLaunchKernelGGL(aq_k_ci_predstats, dim3((unsigned)h->p_kept), dim3(256), 0, 0, h->Xs.get(), cb.B.get(), cb.mpad.get(), h->n, nb,
                     cb.vg.get(), cb.cgv.get(), cb.vw.get(), cb.pok.get(), cb.tol.get());
  if (qa > 0)
    hipLaunchKernelGGL(aq_k_ci_traits, dim3((unsigned)qa), dim3(256), 0, 0, h->Yc.get(), b.order.get(), cb.B.get(), h->n, nb, b.Yo.get(),
                       b.syy.get());
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

// the kernels of one scan after the statistics, in the launch sequence of aq_cis_host.h without the column sums: the tile
// kernel and the reduction of the bests.  Asynchronous.
static int aq_ci_launch_scan(aq_prep *h, AqCiBuf &cb) {
  return aq_cis_launch_scan(h, cb.b, false, [&](unsigned W, const aq_cis_args &a) {
    aq_ci_args ca{};
    ca.c = a;
    ca.mpad = cb.mpad.get(); ca.syy0 = cb.syy0.get(); ca.vg = cb.vg.get(); ca.cgv = cb.cgv.get(); ca.vw = cb.vw.get();
    ca.pok = cb.pok.get(); ca.nb = cb.pl.n_basis;
    aq_screen_a16(h->n, [&](auto a16) { hipLaunchKernelGGL((aq_k_ci_tile<decltype(a16)::value>), dim3(W), dim3(256), 0, 0, ca); });
  });
}

extern "C" int aq_prep_cis_int(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const double *basis, int32_t n_basis,
                               const double *mult, const double *r2_cut, int64_t cap, int32_t *snp, int32_t *trait, double *r,
                               int64_t *n_pairs, int32_t *best_snp, double *best_r, int64_t *n_undef, double *int_tol,
                               aq_cisint_plan *plan_out) {
  if (!s_lo || !s_hi || !basis || !mult || !r2_cut) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_int: NULL s_lo, s_hi, basis, mult or r2_cut");
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_int: NULL handle");
  if (cap < 0) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_int: cap >= 0 required, " + std::to_string(cap) + " given");
  AQ_TRY(aq_ci_check(h, s_lo, s_hi, basis, n_basis, mult, "aq_prep_cis_int"));
  AQ_TRY(aq_screen_need_cut(r2_cut, h->q, "aq_prep_cis_int"));
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_cis_int"));
  AqCiBuf cb;
  AQ_TRY(aq_ci_setup(h, s_lo, s_hi, basis, n_basis, mult, r2_cut, cap, "aq_prep_cis_int", &cb));
  if (plan_out) *plan_out = cb.pl;
  AQ_TRY(aq_ci_launch_stats(h, cb));
  AQ_TRY(aq_ci_launch_scan(h, cb));
  AQ_TRY(aq_cis_copy_scan(h, cb.b, snp, trait, r, n_pairs, best_snp, best_r, n_undef));
  if (int_tol) AQ_HIP(hipMemcpy(int_tol, cb.tol.get(), (size_t)h->p_kept * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}

// Timing hook, after aq_prep_cis_cond_time: the per-predictor kernel and the trait residuals `reps` times between two events,
// then the rest of one scan (the tile kernel, the reduction of the bests), counting only (cap = 0), with the cutoff
// aq_screen_time_cut at df = n - n_basis - 2.
extern "C" int aq_prep_cis_int_time(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const double *basis, int32_t n_basis,
                                    const double *mult, int32_t reps, double *ms_stats, double *ms_scan, aq_cisint_plan *plan_out) {
  if (!s_lo || !s_hi || !basis || !mult || !ms_stats || !ms_scan) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_int_time: NULL argument");
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_int_time: NULL handle");
  if (reps < 1) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_int_time: reps >= 1 required");
  AQ_TRY(aq_ci_check(h, s_lo, s_hi, basis, n_basis, mult, "aq_prep_cis_int_time"));
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_cis_int_time"));
  AqCiBuf cb;
  AQ_TRY(aq_ci_setup(h, s_lo, s_hi, basis, n_basis, mult, nullptr, 0, "aq_prep_cis_int_time", &cb));
  if (plan_out) *plan_out = cb.pl;
  AQ_TRY(aq_cis_upload_time_cut(cb.b, [&](size_t) { return h->n - n_basis - 2; }));
  AQ_TRY(aq_time_launches(reps, ms_stats, [&] { return aq_ci_launch_stats(h, cb); }));
  AQ_TRY(aq_time_launches(reps, ms_scan, [&] { return aq_ci_launch_scan(h, cb); }));
  return AQ_OK;
}
