// aq_prep_cis_cond.hip -- the conditional cis scan of a finished prepare handle (include/atlasqtl_hip.h): aq_prep_cis_cond
// tests every trait against the predictors of its own window after the trait's own conditioning variants have been regressed
// out of both (aq_ciscond_kernels.h; plan by aq_ciscond_plan.h on top of aq_cis_plan.h) and returns what aq_prep_cis returns,
// and k_eff; aq_prep_cis_cond_time times the kernels alone, aq_ciscond_plan_query runs the planner on the host.  The kernels
// are plain HIP that issues no hand-written load: the ISA proof of the look-ahead sweep units does not cover them and need not.
#include "aq_cis_host.h"          // AqCisBuf, aq_cis_setup_complete, aq_cis_keep_syy, aq_cis_launch_scan, aq_cis_launch_tile,
                                  // aq_cis_upload_time_cut, aq_cis_copy_scan, aq_cis_need_windows; aq_screen_host.h
#include "aq_ciscond_kernels.h"   // aq_k_cc_basis, aq_k_cc_tile; aq_ciscond_make_plan, aq_ciscond_check_lists

extern "C" int aq_ciscond_plan_query(int32_t n, int32_t p1, int32_t q, int32_t ncu, const int32_t *s_lo, const int32_t *s_hi,
                                     const int32_t *cond_ptr, aq_ciscond_plan *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_ciscond_plan_query: NULL argument");
  *out = aq_ciscond_plan{};
  std::string err;
  const int rc = aq_ciscond_make_plan(n, p1, q, ncu, s_lo, s_hi, cond_ptr, nullptr, "aq_ciscond_plan_query", out, nullptr, &err);
  if (rc != AQ_OK) *out = aq_ciscond_plan{};
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

// what the conditioning adds to the buffers of a scan
struct AqCcBuf {
  AqCisBuf b;
  AqDev<double> Qo, syy0;
  AqDev<int32_t> ck, cidx, keff_o, keff_t, tile_k;
  aq_ciscond_plan pl{};
};

// the arguments every entry checks before any device call, in the order of the header
static int aq_cc_check(aq_prep *h, const int32_t *s_lo, const int32_t *s_hi, const int32_t *cond_ptr, const int32_t *cond_idx,
                       const char *who) {
  const std::string w(who);
  if (!s_lo || !s_hi || !cond_ptr || !cond_idx) return aq_fail(AQ_ERR_ARG, w + ": NULL s_lo, s_hi, cond_ptr or cond_idx");
  if (!h) return aq_fail(AQ_ERR_ARG, w + ": NULL handle");
  std::string err;
  const int rc = aq_ciscond_check_lists(cond_ptr, cond_idx, h->q, h->p_kept, AQ_ERR_ARG, who, &err);
  if (rc != AQ_OK) return aq_fail(rc, err);
  return aq_cis_need_windows(h, s_lo, s_hi, who);
}

// the complete-Y set-up of aq_cis_host.h, the plan, and the lists in the order
static int aq_cc_setup(aq_prep *h, const int32_t *s_lo, const int32_t *s_hi, const int32_t *cond_ptr, const int32_t *cond_idx,
                       const double *r2_cut, int64_t cap, const char *who, AqCcBuf *cb) {
  AqCisBuf &b = cb->b;
  AQ_TRY(aq_cis_setup_complete(h, s_lo, s_hi, r2_cut, cap, who, "conditional", &b));
  std::string err;
  // the cis plan inside is the same pure function of the same arguments as b.pl, and its order and work list are b.wk
  const int rc = aq_ciscond_make_plan(h->n, h->p_kept, h->q, b.ncu, s_lo, s_hi, cond_ptr, cond_idx, who, &cb->pl, nullptr, &err);
  if (rc != AQ_OK) return aq_fail(rc, err);
  const size_t qa = (size_t)b.wk.q_active, n = (size_t)h->n, q = (size_t)h->q;
  const int kc = cb->pl.kc;
  std::vector<int32_t> ck(qa), cidx(qa * AQ_CISCOND_KMAX, 0);
  for (size_t j = 0; j < qa; j++) {
    const int t = b.wk.order[j];
    ck[j] = cond_ptr[t + 1] - cond_ptr[t];
    for (int c = 0; c < ck[j]; c++) cidx[j * AQ_CISCOND_KMAX + (size_t)c] = cond_idx[cond_ptr[t] + c];
  }
  AQ_TRY(aq_cis_upload(&cb->ck, ck));
  AQ_TRY(aq_cis_upload(&cb->cidx, cidx));
  AQ_TRY(cb->Qo.alloc(kc > 0 && qa > 0 ? (size_t)kc * qa * n : 1));
  AQ_TRY(cb->keff_o.alloc(qa > 0 ? qa : 1));
  AQ_TRY(cb->keff_t.alloc(q));
  AQ_TRY(cb->tile_k.alloc(b.pl.trait_tiles > 0 ? (size_t)b.pl.trait_tiles : 1));
  return aq_cis_keep_syy(b, &cb->syy0);     // the basis kernel overwrites b.syy with S~yy_t
}

// the basis kernel, then the largest k_eff per trait tile: one small copy back, the tile kernel's grid does not depend on it
static int aq_cc_launch_basis(aq_prep *h, AqCcBuf &cb) {
  AqCisBuf &b = cb.b;
  const int qa = b.wk.q_active;
  AQ_HIP(hipMemsetAsync(cb.keff_t.get(), 0, (size_t)h->q * sizeof(int32_t), 0));
  if (qa > 0) {
    hipLaunchKernelGGL(aq_k_cc_basis, dim3((unsigned)qa), dim3(256), 0, 0, h->Xs.get(), h->Yc.get(), b.order.get(), cb.ck.get(),
                       cb.cidx.get(), cb.syy0.get(), h->n, qa, cb.pl.kc, cb.Qo.get(), b.Yo.get(), b.syy.get(), cb.keff_o.get(),
                       cb.keff_t.get());
    AQ_HIP(hipGetLastError());
  }
  return AQ_OK;
}

static int aq_cc_tile_k(AqCcBuf &cb) {
  AqCisBuf &b = cb.b;
  const size_t qa = (size_t)b.wk.q_active, tiles = (size_t)b.pl.trait_tiles;
  if (tiles == 0) return AQ_OK;
  std::vector<int32_t> keff(qa), tk(tiles, 0);
  AQ_HIP(hipMemcpy(keff.data(), cb.keff_o.get(), qa * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (size_t j = 0; j < qa; j++) tk[j / AQ_CIS_TILE] = std::max(tk[j / AQ_CIS_TILE], keff[j]);
  AQ_HIP(hipMemcpy(cb.tile_k.get(), tk.data(), tiles * sizeof(int32_t), hipMemcpyHostToDevice));
  return AQ_OK;
}

template <int KC>
static void aq_cc_launch_tile(unsigned grid, const aq_cc_args &ca) {
  aq_screen_a16(ca.c.n, [&](auto a16) { hipLaunchKernelGGL((aq_k_cc_tile<KC, decltype(a16)::value>), dim3(grid), dim3(256), 0, 0, ca); });
}

// the kernels of one scan after the basis, in the launch sequence of aq_cis_host.h: the column sums, the tile kernel of the
// plan's KC (the plain scan's for KC = 0, on the copies of y that the basis kernel made), the reduction of the bests.
// Asynchronous.
static int aq_cc_launch_scan(aq_prep *h, AqCcBuf &cb) {
  return aq_cis_launch_scan(h, cb.b, true, [&](unsigned W, const aq_cis_args &a) {
    aq_cc_args ca{};
    ca.c = a;
    ca.Qo = cb.Qo.get(); ca.syy0 = cb.syy0.get(); ca.keff = cb.keff_o.get(); ca.tile_k = cb.tile_k.get();
    switch (cb.pl.kc) {
      case 0: aq_cis_launch_tile<false>(W, ca.c); break;   // no list: S~yy = Syy and k_eff = 0 everywhere, the plain scan's kernel
      case 1: aq_cc_launch_tile<1>(W, ca); break;
      case 2: aq_cc_launch_tile<2>(W, ca); break;
      default: aq_cc_launch_tile<4>(W, ca); break;
    }
  });
}

extern "C" int aq_prep_cis_cond(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const int32_t *cond_ptr, const int32_t *cond_idx,
                                const double *r2_cut, int64_t cap, int32_t *snp, int32_t *trait, double *r, int64_t *n_pairs,
                                int32_t *best_snp, double *best_r, int64_t *n_undef, int32_t *k_eff, aq_ciscond_plan *plan_out) {
  if (!r2_cut) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_cond: NULL r2_cut");
  if (cap < 0) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_cond: cap >= 0 required, " + std::to_string(cap) + " given");
  AQ_TRY(aq_cc_check(h, s_lo, s_hi, cond_ptr, cond_idx, "aq_prep_cis_cond"));
  AQ_TRY(aq_screen_need_cut(r2_cut, h->q, "aq_prep_cis_cond"));
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_cis_cond"));
  const size_t q = (size_t)h->q;
  AqCcBuf cb;
  AQ_TRY(aq_cc_setup(h, s_lo, s_hi, cond_ptr, cond_idx, r2_cut, cap, "aq_prep_cis_cond", &cb));
  if (plan_out) *plan_out = cb.pl;
  AQ_TRY(aq_cc_launch_basis(h, cb));
  AQ_TRY(aq_cc_tile_k(cb));
  AQ_TRY(aq_cc_launch_scan(h, cb));
  AQ_TRY(aq_cis_copy_scan(h, cb.b, snp, trait, r, n_pairs, best_snp, best_r, n_undef));
  if (k_eff) AQ_HIP(hipMemcpy(k_eff, cb.keff_t.get(), q * sizeof(int32_t), hipMemcpyDeviceToHost));
  return AQ_OK;
}

// Timing hook, after aq_prep_cis_time: the basis kernel `reps` times between two events, then the scan's kernels (column
// sums, tile kernel of the plan's KC, reduction of the bests), counting only (cap = 0), with the cutoff aq_screen_time_cut at
// df_t = n - 2 - n_cov - k_eff[t].
extern "C" int aq_prep_cis_cond_time(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const int32_t *cond_ptr,
                                     const int32_t *cond_idx, int32_t reps, double *ms_basis, double *ms_scan, aq_ciscond_plan *plan_out) {
  if (!ms_basis || !ms_scan) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_cond_time: NULL argument");
  if (reps < 1) return aq_fail(AQ_ERR_ARG, "aq_prep_cis_cond_time: reps >= 1 required");
  AQ_TRY(aq_cc_check(h, s_lo, s_hi, cond_ptr, cond_idx, "aq_prep_cis_cond_time"));
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_cis_cond_time"));
  AqCcBuf cb;
  AQ_TRY(aq_cc_setup(h, s_lo, s_hi, cond_ptr, cond_idx, nullptr, 0, "aq_prep_cis_cond_time", &cb));
  if (plan_out) *plan_out = cb.pl;
  AQ_TRY(aq_time_launches(reps, ms_basis, [&] { return aq_cc_launch_basis(h, cb); }));
  AQ_TRY(aq_cc_tile_k(cb));
  {
    AqCisBuf &b = cb.b;
    const size_t qa = (size_t)b.wk.q_active;
    std::vector<int32_t> keff(qa);
    if (qa > 0) AQ_HIP(hipMemcpy(keff.data(), cb.keff_o.get(), qa * sizeof(int32_t), hipMemcpyDeviceToHost));
    AQ_TRY(aq_cis_upload_time_cut(b, [&](size_t j) { return h->n - 2 - h->n_cov - keff[j]; }));
  }
  AQ_TRY(aq_time_launches(reps, ms_scan, [&] { return aq_cc_launch_scan(h, cb); }));
  return AQ_OK;
}
