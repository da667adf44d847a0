// aq_prep_marginal.hip -- the marginal screen of a finished prepare handle (include/atlasqtl_hip.h): aq_prep_marginal tests
// every predictor of the handle's current matrix against every trait on the f64 matrix pipe (aq_mscreen_kernels.h, planned by
// aq_mscreen_plan.h) and returns the selected pairs, the per-predictor counts and each trait's best predictor;
// aq_prep_marginal_time times the kernels alone, aq_mscreen_plan_query runs the planner on the host.  The kernels are plain HIP
// that issues no hand-written load: the ISA proof of the look-ahead sweep units does not cover them and need not.
#include "aq_screen_host.h"      // aq_screen_*; aq_prep.h, aq_internal.h; aq_screen_tile.h: aq_k_ms_traitstats, aq_k_ms_colstats
#include "aq_mscreen_kernels.h"  // aq_k_ms_tile, aq_k_ms_best; aq_mscreen_make_plan

extern "C" int aq_mscreen_plan_query(int32_t n, int32_t p1, int32_t q, int32_t masked, int32_t ncu, aq_mscreen_plan *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_mscreen_plan_query: NULL argument");
  *out = aq_mscreen_plan{};
  std::string err;
  const int rc = aq_mscreen_make_plan(n, p1, q, masked, ncu, 0, "aq_mscreen_plan_query", out, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

// the device side of one screen: the per-trait and per-predictor sums, the counters, the table and the partial bests
struct AqMsBuf {
  AqDev<double> cut, sx, sxx, syy, part_r, best_r, r, dense;
  AqDev<int> mt;
  AqDev<int32_t> part_s, best_s, snp, trait;
  AqDev<unsigned long long> counters, rs;    // counters: n_pairs, n_undefined
  std::vector<int> mt_host;
  aq_mscreen_plan pl{};
  int64_t cap = 0;
  bool want_dense = false;
};

// Syy_t and m_t of the handle's traits, whether any value is missing, and from that the plan; then every buffer
static int aq_ms_setup(aq_prep *h, int64_t cap, bool want_dense, const char *who, AqMsBuf *b) {
  const size_t p1 = (size_t)h->p_kept, q = (size_t)h->q;
  int masked = 0, ncu = 0;
  AQ_TRY(aq_screen_trait_stats(h, &b->syy, &b->mt, &b->mt_host, &masked, &ncu));
  std::string err;
  const int rc = aq_mscreen_make_plan(h->n, h->p_kept, h->q, masked, ncu, aq_screen_env("AQ_MSCREEN_TILE"), who, &b->pl, &err);
  if (rc != AQ_OK) return aq_fail(rc, err);
  b->cap = cap;
  b->want_dense = want_dense;
  AQ_TRY(b->cut.alloc(q));
  if (!masked) {
    AQ_TRY(b->sx.alloc(p1));
    AQ_TRY(b->sxx.alloc(p1));
  }
  AQ_TRY(b->counters.alloc(2));
  AQ_TRY(b->rs.alloc(p1));
  AQ_TRY(b->part_r.alloc((size_t)b->pl.tiles_p * q));
  AQ_TRY(b->part_s.alloc((size_t)b->pl.tiles_p * q));
  AQ_TRY(b->best_r.alloc(q));
  AQ_TRY(b->best_s.alloc(q));
  if (cap > 0) {
    AQ_TRY(b->snp.alloc((size_t)cap));
    AQ_TRY(b->trait.alloc((size_t)cap));
    AQ_TRY(b->r.alloc((size_t)cap));
  }
  if (want_dense) AQ_TRY(b->dense.alloc(p1 * q));
  return AQ_OK;
}

template <int T, bool MASKED>
static void aq_ms_launch_tile(unsigned grid, const aq_ms_args &a) {
  aq_screen_a16(a.n, [&](auto a16) { hipLaunchKernelGGL((aq_k_ms_tile<T, MASKED, decltype(a16)::value>), dim3(grid), dim3(256), 0, 0, a); });
}

// every kernel of one screen after aq_ms_setup, with b->cut holding the cutoffs.  Asynchronous.
static int aq_ms_launch(aq_prep *h, AqMsBuf &b) {
  const int p1 = h->p_kept, q = h->q;
  AQ_HIP(hipMemsetAsync(b.counters.get(), 0, 2 * sizeof(unsigned long long), 0));
  AQ_HIP(hipMemsetAsync(b.rs.get(), 0, (size_t)p1 * sizeof(unsigned long long), 0));
  if (!b.pl.masked) hipLaunchKernelGGL(aq_k_ms_colstats, dim3((unsigned)p1), dim3(256), 0, 0, h->Xs.get(), h->n, b.sx.get(), b.sxx.get());
  aq_ms_args a{};
  a.Xs = h->Xs.get(); a.Yc = h->Yc.get();
  a.n = h->n; a.p1 = p1; a.q = q; a.n_cov = h->n_cov; a.tiles_p = b.pl.tiles_p;
  a.sx = b.sx.get(); a.sxx = b.sxx.get(); a.syy = b.syy.get(); a.mt = b.mt.get(); a.cut = b.cut.get();
  a.snp = b.snp.get(); a.trait = b.trait.get(); a.r = b.r.get(); a.cap = (long long)b.cap;
  a.n_pairs = b.counters.get(); a.n_undef = b.counters.get() + 1; a.rs = b.rs.get();
  a.part_r = b.part_r.get(); a.part_s = b.part_s.get();
  a.r_dense = b.want_dense ? b.dense.get() : nullptr;
  const unsigned grid = (unsigned)b.pl.n_tiles;
  if (b.pl.masked)
    aq_ms_launch_tile<AQ_MSCREEN_TILE_MASKED, true>(grid, a);
  else if (b.pl.tile == 128)
    aq_ms_launch_tile<128, false>(grid, a);
  else
    aq_ms_launch_tile<64, false>(grid, a);
  hipLaunchKernelGGL(aq_k_ms_best, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, 0, b.part_r.get(), b.part_s.get(), b.pl.tiles_p, q,
                     b.best_s.get(), b.best_r.get());
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

extern "C" int aq_prep_marginal(aq_prep_handle h, const double *r2_cut, int64_t cap, int32_t *snp, int32_t *trait, double *r,
                                int64_t *n_pairs, int64_t *rs, int32_t *best_snp, double *best_r, int64_t *n_undefined, double *r_dense) {
  if (!r2_cut) return aq_fail(AQ_ERR_ARG, "aq_prep_marginal: NULL r2_cut");
  if (cap < 0) return aq_fail(AQ_ERR_ARG, "aq_prep_marginal: cap >= 0 required, " + std::to_string(cap) + " given");
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_marginal: NULL handle");
  AQ_TRY(aq_screen_need_cut(r2_cut, h->q, "aq_prep_marginal"));
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_marginal"));
  const size_t p1 = (size_t)h->p_kept, q = (size_t)h->q;
  AqMsBuf b;
  AQ_TRY(aq_ms_setup(h, cap, r_dense != nullptr, "aq_prep_marginal", &b));
  AQ_HIP(hipMemcpy(b.cut.get(), r2_cut, q * sizeof(double), hipMemcpyHostToDevice));
  AQ_TRY(aq_ms_launch(h, b));
  unsigned long long cnt[2] = {0, 0};
  AQ_HIP(hipMemcpy(cnt, b.counters.get(), sizeof(cnt), hipMemcpyDeviceToHost));
  if (n_pairs) *n_pairs = (int64_t)cnt[0];
  if (n_undefined) *n_undefined = (int64_t)cnt[1];
  AQ_TRY(aq_screen_copy_pairs(cnt[0], cap, b.snp, b.trait, b.r, snp, trait, r));
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
  if (rs) AQ_HIP(hipMemcpy(rs, b.rs.get(), p1 * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (best_snp) AQ_HIP(hipMemcpy(best_snp, b.best_s.get(), q * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (best_r) AQ_HIP(hipMemcpy(best_r, b.best_r.get(), q * sizeof(double), hipMemcpyDeviceToHost));
  if (r_dense) AQ_HIP(hipMemcpy(r_dense, b.dense.get(), p1 * q * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}

// Timing hook of aq_prep_marginal: every kernel of one screen, `reps` times between two events, counting only, without the
// copies.  The cutoff is aq_screen_time_cut at df_t = m_t - 2 - n_cov.
extern "C" int aq_prep_marginal_time(aq_prep_handle h, int32_t reps, double *ms_per_call, aq_mscreen_plan *plan_out) {
  if (!h || !ms_per_call) return aq_fail(AQ_ERR_ARG, "aq_prep_marginal_time: NULL argument");
  if (reps < 1) return aq_fail(AQ_ERR_ARG, "aq_prep_marginal_time: reps >= 1 required");
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_marginal_time"));
  const size_t q = (size_t)h->q;
  AqMsBuf b;
  AQ_TRY(aq_ms_setup(h, 0, false, "aq_prep_marginal_time", &b));
  if (plan_out) *plan_out = b.pl;
  std::vector<double> cut(q);
  for (size_t t = 0; t < q; t++) cut[t] = aq_screen_time_cut(b.mt_host[t] - 2 - h->n_cov);
  AQ_HIP(hipMemcpy(b.cut.get(), cut.data(), q * sizeof(double), hipMemcpyHostToDevice));
  return aq_time_launches(reps, ms_per_call, [&] { return aq_ms_launch(h, b); });
}
