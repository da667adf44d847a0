// aq_cis_host.h -- the host side that the entries of the cis scan share (aq_prep_cis.hip: the plain scan and its permutation
// nulls; aq_prep_cis_cond.hip: the conditional scan; aq_prep_cis_int.hip: the interaction scan): the device buffers of one call, the set-up that runs the planner of
// aq_cis_plan.h and uploads the order, the work list and the per-trait arrays, the arguments every tile kernel takes, and
// the column sums, the launch of the plain scan's tile kernel and the copy-back of a scan's outputs.  Moved here from the three
// units, which each had a copy: aq_cis_launch_scan, aq_cis_upload_time_cut, aq_cis_setup_complete and aq_cis_keep_syy.  What the
// marginal screen's entries need as well lies beneath, in aq_screen_host.h.  Static functions: each unit has its own copy.
#pragma once
#include "aq_screen_host.h"   // aq_screen_*; aq_prep.h, aq_internal.h
#include "aq_cis_kernels.h"   // aq_k_cis_*; aq_screen_tile.h: aq_k_ms_gather, aq_k_ms_colstats; aq_cis_make_plan

// the device side of one call: what does not change with the permutation, the scan's outputs, and the buffers of one launch of
// permutations
struct AqCisBuf {
  AqDev<double> Yo, sx, sxx, syy, cut, part_r, best_r, r, Yp, max_r2;
  AqDev<int> mt;
  AqDev<int32_t> order, lo, hi, first_item, item_tile, item_p0, part_s, best_s, snp, trait, perm;
  AqDev<unsigned long long> counter, undef, key;
  std::vector<int> mt_host;                  // m_t per ordered trait with a window
  aq_cis_plan pl{};
  aq_cis_work wk;
  int64_t cap = 0;
  int ncu = 0;                               // the CU count the plan was made for
};

template <typename T>
static int aq_cis_upload(AqDev<T> *dst, const std::vector<T> &src) {
  AQ_TRY(dst->alloc(src.size() > 0 ? src.size() : 1));
  if (!src.empty()) AQ_HIP(hipMemcpy(dst->get(), src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return AQ_OK;
}

// Syy_t and m_t of the handle's traits, whether any value is missing (over ALL traits, as aq_prep_marginal decides it, so
// that the same instance computes the same bits), the plan, the order and the work list; the per-trait arrays in the order;
// the buffers of the scan (scan) and of one launch of permutations (n_perm > 0).  r2_cut may be NULL (the *_time entry sets
// its own, the permutations use none).
static int aq_cis_setup(aq_prep *h, const int32_t *s_lo, const int32_t *s_hi, const double *r2_cut, int64_t cap, bool scan, int n_perm,
                        const char *who, AqCisBuf *b) {
  const size_t p1 = (size_t)h->p_kept, q = (size_t)h->q, n = (size_t)h->n;
  std::vector<double> syy(q);
  std::vector<int> mt;
  int masked = 0, ncu = 0;
  {
    AqDev<double> dsyy;                      // by the trait's own index: the buffers of the call hold the ordered ones
    AqDev<int> dmt;
    AQ_TRY(aq_screen_trait_stats(h, &dsyy, &dmt, &mt, &masked, &ncu));
    AQ_HIP(hipMemcpy(syy.data(), dsyy.get(), q * sizeof(double), hipMemcpyDeviceToHost));
  }
  std::string err;
  const int rc = aq_cis_make_plan(h->n, h->p_kept, h->q, masked, ncu, s_lo, s_hi, n_perm, n_perm > 0 ? aq_screen_env("AQ_CIS_PB") : 0,
                                  n_perm > 0 ? aq_screen_env("AQ_CIS_BATCH") : 0, who, &b->pl, &b->wk, &err);
  if (rc != AQ_OK) return aq_fail(rc, err);
  const size_t qa = (size_t)b->wk.q_active, W = (size_t)b->pl.n_items;
  b->cap = cap;
  b->ncu = ncu;
  {
    std::vector<double> syy_o(qa), cut_o(qa);
    std::vector<int32_t> lo_o(qa), hi_o(qa);
    b->mt_host.resize(qa);
    for (size_t j = 0; j < qa; j++) {
      const size_t t = (size_t)b->wk.order[j];
      syy_o[j] = syy[t];
      b->mt_host[j] = mt[t];
      cut_o[j] = r2_cut ? r2_cut[t] : std::numeric_limits<double>::infinity();
      lo_o[j] = s_lo[t];
      hi_o[j] = s_hi[t];
    }
    AQ_TRY(aq_cis_upload(&b->syy, syy_o));
    AQ_TRY(aq_cis_upload(&b->mt, b->mt_host));
    AQ_TRY(aq_cis_upload(&b->cut, cut_o));
    AQ_TRY(aq_cis_upload(&b->lo, lo_o));
    AQ_TRY(aq_cis_upload(&b->hi, hi_o));
  }
  AQ_TRY(aq_cis_upload(&b->order, b->wk.order));
  AQ_TRY(aq_cis_upload(&b->first_item, b->wk.first_item));
  AQ_TRY(aq_cis_upload(&b->item_tile, b->wk.item_tile));
  AQ_TRY(aq_cis_upload(&b->item_p0, b->wk.item_p0));
  if (!masked) {
    AQ_TRY(b->sx.alloc(p1));
    AQ_TRY(b->sxx.alloc(p1));
  }
  if (scan) {
    AQ_TRY(b->Yo.alloc(qa > 0 ? qa * n : 1));
    AQ_TRY(b->counter.alloc(1));
    AQ_TRY(b->undef.alloc(q));
    AQ_TRY(b->part_r.alloc(W > 0 ? W * AQ_CIS_TILE : 1));
    AQ_TRY(b->part_s.alloc(W > 0 ? W * AQ_CIS_TILE : 1));
    AQ_TRY(b->best_r.alloc(q));
    AQ_TRY(b->best_s.alloc(q));
    if (cap > 0) {
      AQ_TRY(b->snp.alloc((size_t)cap));
      AQ_TRY(b->trait.alloc((size_t)cap));
      AQ_TRY(b->r.alloc((size_t)cap));
    }
  }
  if (n_perm > 0) {
    const size_t batch = (size_t)b->pl.batch;
    AQ_TRY(b->Yp.alloc(batch * (qa > 0 ? qa : 1) * n));
    AQ_TRY(b->perm.alloc(batch * n));
    AQ_TRY(b->key.alloc(batch * q));
    AQ_TRY(b->max_r2.alloc(batch * q));
  }
  return AQ_OK;
}

// aq_cis_setup for a scan that takes complete Y only: missing values are refused under the entry's name, `scan` naming the scan
static int aq_cis_setup_complete(aq_prep *h, const int32_t *s_lo, const int32_t *s_hi, const double *r2_cut, int64_t cap, const char *who,
                                 const char *scan, AqCisBuf *b) {
  AQ_TRY(aq_cis_setup(h, s_lo, s_hi, r2_cut, cap, true, 0, who, b));
  if (b->pl.masked)
    return aq_fail(AQ_ERR_UNSUPPORTED, std::string(who) + ": Y has missing values; the " + scan + " scan takes complete Y only");
  return AQ_OK;
}

// b.syy holds Syy_t per ordered trait; a scan whose first kernel overwrites it keeps the trait's own in syy0 first
static int aq_cis_keep_syy(AqCisBuf &b, AqDev<double> *syy0) {
  const size_t qa = (size_t)b.wk.q_active;
  AQ_TRY(syy0->alloc(qa > 0 ? qa : 1));
  if (qa > 0) AQ_HIP(hipMemcpy(syy0->get(), b.syy.get(), qa * sizeof(double), hipMemcpyDeviceToDevice));
  return AQ_OK;
}

// the timing hooks' cutoff per ordered trait j: aq_screen_time_cut at df(j) degrees of freedom, in the place of r2_cut
template <typename Df>
static int aq_cis_upload_time_cut(AqCisBuf &b, Df &&df) {
  const size_t qa = (size_t)b.wk.q_active;
  std::vector<double> cut(qa);
  for (size_t j = 0; j < qa; j++) cut[j] = aq_screen_time_cut(df(j));
  if (qa > 0) AQ_HIP(hipMemcpy(b.cut.get(), cut.data(), qa * sizeof(double), hipMemcpyHostToDevice));
  return AQ_OK;
}

static aq_cis_args aq_cis_common_args(aq_prep *h, AqCisBuf &b) {
  aq_cis_args a{};
  a.Xs = h->Xs.get();
  a.n = h->n; a.p1 = h->p_kept; a.q = h->q; a.qa = b.wk.q_active; a.n_cov = h->n_cov; a.W = (int)b.pl.n_items;
  a.item_tile = b.item_tile.get(); a.item_p0 = b.item_p0.get();
  a.sx = b.sx.get(); a.sxx = b.sxx.get(); a.syy = b.syy.get(); a.cut = b.cut.get(); a.mt = b.mt.get();
  a.lo = b.lo.get(); a.hi = b.hi.get(); a.orig = b.order.get();
  return a;
}

// the arguments of a scan over the ordered traits in b.Yo: the common ones and the scan's outputs
static aq_cis_args aq_cis_scan_args(aq_prep *h, AqCisBuf &b) {
  aq_cis_args a = aq_cis_common_args(h, b);
  a.Yo = b.Yo.get();
  a.nb = 1;
  a.snp = b.snp.get(); a.trait = b.trait.get(); a.r = b.r.get(); a.cap = (long long)b.cap;
  a.n_pairs = b.counter.get(); a.n_undef = b.undef.get();
  a.part_r = b.part_r.get(); a.part_s = b.part_s.get();
  return a;
}

// the plain scan's tile kernel over the W work items (the conditional scan runs it where no trait has a list)
template <bool MASKED>
static void aq_cis_launch_tile(unsigned W, const aq_cis_args &a) {
  aq_screen_a16(a.n, [&](auto a16) { hipLaunchKernelGGL((aq_k_cis_tile<MASKED, decltype(a16)::value>), dim3(W), dim3(256), 0, 0, a); });
}

// what every scan returns, after its kernels: the number of selected pairs and their table, each trait's best predictor and
// its undefined pairs
static int aq_cis_copy_scan(aq_prep *h, AqCisBuf &b, int32_t *snp, int32_t *trait, double *r, int64_t *n_pairs, int32_t *best_snp,
                            double *best_r, int64_t *n_undef) {
  const size_t q = (size_t)h->q;
  unsigned long long cnt = 0;
  AQ_HIP(hipMemcpy(&cnt, b.counter.get(), sizeof(cnt), hipMemcpyDeviceToHost));
  if (n_pairs) *n_pairs = (int64_t)cnt;
  AQ_TRY(aq_screen_copy_pairs(cnt, b.cap, b.snp, b.trait, b.r, snp, trait, r));
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
  if (best_snp) AQ_HIP(hipMemcpy(best_snp, b.best_s.get(), q * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (best_r) AQ_HIP(hipMemcpy(best_r, b.best_r.get(), q * sizeof(double), hipMemcpyDeviceToHost));
  if (n_undef) AQ_HIP(hipMemcpy(n_undef, b.undef.get(), q * sizeof(int64_t), hipMemcpyDeviceToHost));
  return AQ_OK;
}

// Sx and Sxx of every column for the complete instances.  Asynchronous.
static int aq_cis_colstats(aq_prep *h, AqCisBuf &b) {
  if (!b.pl.masked) {
    hipLaunchKernelGGL(aq_k_ms_colstats, dim3((unsigned)h->p_kept), dim3(256), 0, 0, h->Xs.get(), h->n, b.sx.get(), b.sxx.get());
    AQ_HIP(hipGetLastError());
  }
  return AQ_OK;
}

// every kernel of one scan after its set-up, on the null stream: the counter and the undefined counts zeroed, the column sums
// (colstats), then, if the plan has work items, the unit's tile(W, the scan's arguments), then the bests.  Asynchronous.
template <typename Tile>
static int aq_cis_launch_scan(aq_prep *h, AqCisBuf &b, bool colstats, Tile &&tile) {
  const int q = h->q, qa = b.wk.q_active;
  const unsigned W = (unsigned)b.pl.n_items;
  AQ_HIP(hipMemsetAsync(b.counter.get(), 0, sizeof(unsigned long long), 0));
  AQ_HIP(hipMemsetAsync(b.undef.get(), 0, (size_t)q * sizeof(unsigned long long), 0));
  if (colstats) AQ_TRY(aq_cis_colstats(h, b));
  if (W > 0) tile(W, aq_cis_scan_args(h, b));
  hipLaunchKernelGGL(aq_k_cis_best, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, 0, b.part_r.get(), b.part_s.get(), b.first_item.get(),
                     b.order.get(), qa, q, b.best_s.get(), b.best_r.get());
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

// the window checks that need the handle's p1 and q, under the entry's name
static int aq_cis_need_windows(aq_prep *h, const int32_t *s_lo, const int32_t *s_hi, const char *who) {
  std::string err;
  const int rc = aq_cis_check_windows(s_lo, s_hi, h->q, h->p_kept, who, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}
