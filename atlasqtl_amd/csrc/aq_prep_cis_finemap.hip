// aq_prep_cis_finemap.hip -- cis fine-mapping of a finished prepare handle (include/atlasqtl_hip.h): aq_prep_cis_finemap fits
// SuSiE per trait over the predictors of its own window by IBSS, all traits of a batch in lockstep (aq_finemap_kernels.h; plan
// by aq_finemap_plan.h on top of aq_cis_plan.h), and returns the rows of alpha above each trait's threshold and the per-trait
// scalars; aq_prep_set_purity gives the purity of credible sets; aq_prep_cis_finemap_time times the four kernels of one
// iteration, aq_finemap_plan_query runs the planner on the host.  The kernels are plain HIP that issues no hand-written load:
// the ISA proof of the look-ahead sweep units does not cover them and need not.
#include "aq_cis_host.h"          // AqCisBuf, aq_cis_setup_complete, aq_cis_colstats, aq_cis_upload, aq_cis_need_windows; aq_screen_host.h
#include "aq_finemap_kernels.h"   // aq_k_fm_*; aq_finemap_make_plan

extern "C" int aq_finemap_plan_query(int32_t n, int32_t p1, int32_t q, int32_t ncu, const int32_t *s_lo, const int32_t *s_hi, int32_t L,
                                     aq_finemap_plan *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_finemap_plan_query: NULL argument");
  *out = aq_finemap_plan{};
  std::string err;
  const int rc = aq_finemap_make_plan(n, p1, q, ncu, s_lo, s_hi, L, aq_screen_env("AQ_FM_BATCH_TILES"), "aq_finemap_plan_query", out,
                                      nullptr, &err);
  if (rc != AQ_OK) *out = aq_finemap_plan{};
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

static int aq_fm_check_params(const aq_finemap_params *pm, const char *who) {
  const std::string w(who);
  if (!pm) return aq_fail(AQ_ERR_ARG, w + ": NULL params");
  if (pm->L < 1 || pm->L > AQ_FM_LMAX)
    return aq_fail(AQ_ERR_ARG, w + ": L must lie in [1, " + std::to_string(AQ_FM_LMAX) + "], " + std::to_string(pm->L) + " given");
  if (pm->max_iter < 1) return aq_fail(AQ_ERR_ARG, w + ": max_iter >= 1 required");
  if (!(pm->tol >= 0.0) || !std::isfinite(pm->tol)) return aq_fail(AQ_ERR_ARG, w + ": tol must be finite and >= 0");
  if (!(pm->scaled_prior_variance > 0.0) || !std::isfinite(pm->scaled_prior_variance))
    return aq_fail(AQ_ERR_ARG, w + ": scaled_prior_variance must be finite and > 0");
  if (!(pm->coverage > 0.0 && pm->coverage < 1.0)) return aq_fail(AQ_ERR_ARG, w + ": coverage must lie in (0, 1)");
  if (!(pm->alpha_min >= 0.0 && pm->alpha_min <= 1.0)) return aq_fail(AQ_ERR_ARG, w + ": alpha_min must lie in [0, 1]");
  return AQ_OK;
}

// the device side of one call: the set-up of the cis scan, what is kept per ordered trait, and the buffers of one batch
struct AqFmBuf {
  AqCisBuf b;
  aq_finemap_plan pl{};
  AqDev<double> Z, A, M, R, Rf, fit;
  AqDev<double> thr, sig2, sig2_used, elbo_prev, V, V_used, lbf, szam, sdam2, trace;
  AqDev<int> act, P;
  AqDev<int32_t> n_iter, conv, act_items, act_tiles;
  AqDev<int32_t> row_snp, row_trait, row_effect;
  AqDev<double> row_alpha, row_mu, row_mu2;
  AqDev<unsigned long long> n_rows;
  std::vector<int> act_host, P_host;           // per ordered trait
  std::vector<double> d_host;                  // p1
  int max_iter = 0;
};

// the set-up of the cis scan for complete Y, the plan, x'x of every column, per ordered trait the predictors with prior
// weight, the threshold of its rows and whether it is fitted at all (asked for, and a predictor with weight), the start of
// IBSS, and the buffers of the largest batch.  active: by the trait's own index, or NULL for all.
static int aq_fm_setup(aq_prep *h, const int32_t *s_lo, const int32_t *s_hi, const int32_t *active, const aq_finemap_params &pm,
                       int64_t cap, const char *who, AqFmBuf *fb) {
  AqCisBuf &b = fb->b;
  AQ_TRY(aq_cis_setup_complete(h, s_lo, s_hi, nullptr, 0, who, "fine-mapping", &b));
  std::string err;
  // the cis plan inside is the same pure function of the same arguments as b.pl, and its order and work list are b.wk
  const int rc = aq_finemap_make_plan(h->n, h->p_kept, h->q, b.ncu, s_lo, s_hi, pm.L, aq_screen_env("AQ_FM_BATCH_TILES"), who, &fb->pl,
                                      nullptr, &err);
  if (rc != AQ_OK) return aq_fail(rc, err);
  const size_t qa = (size_t)b.wk.q_active, q = (size_t)h->q, p1 = (size_t)h->p_kept, n = (size_t)h->n, L = (size_t)pm.L;
  const size_t qa1 = qa > 0 ? qa : 1;
  AQ_TRY(aq_cis_colstats(h, b));
  fb->d_host.resize(p1);
  AQ_HIP(hipMemcpy(fb->d_host.data(), b.sxx.get(), p1 * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> syy(qa1), thr(qa1, 0.0), sig2(qa1, 0.0), V(L * qa1, 0.0);
  if (qa > 0) AQ_HIP(hipMemcpy(syy.data(), b.syy.get(), qa * sizeof(double), hipMemcpyDeviceToHost));
  fb->act_host.assign(qa1, 0);
  fb->P_host.assign(qa1, 0);
  const double dmin = 1e-10 * (double)n;
  for (size_t j = 0; j < qa; j++) {
    const int t = b.wk.order[j];
    int P = 0;
    for (int s = s_lo[t]; s < s_hi[t]; s++) P += fb->d_host[(size_t)s] > dmin;
    fb->P_host[j] = P;
    fb->act_host[j] = P > 0 && (!active || active[t] != 0);
    thr[j] = P > 0 ? std::min(pm.alpha_min, 0.1 * (1.0 - pm.coverage) / (double)P) : 0.0;
    sig2[j] = syy[j] / (double)(h->n - 1);
    for (size_t l = 0; l < L; l++) V[l * qa + j] = pm.scaled_prior_variance * syy[j] / (double)(h->n - 1);
  }
  AQ_TRY(aq_cis_upload(&fb->act, fb->act_host));
  AQ_TRY(aq_cis_upload(&fb->P, fb->P_host));
  AQ_TRY(aq_cis_upload(&fb->thr, thr));
  AQ_TRY(aq_cis_upload(&fb->sig2, sig2));
  AQ_TRY(aq_cis_upload(&fb->V, V));
  AQ_TRY(aq_cis_upload(&fb->elbo_prev, std::vector<double>(qa1, -std::numeric_limits<double>::infinity())));
  AQ_TRY(fb->sig2_used.alloc_zeroed(qa1));
  AQ_TRY(fb->V_used.alloc_zeroed(L * qa1));
  AQ_TRY(fb->lbf.alloc_zeroed(L * qa1));
  AQ_TRY(fb->szam.alloc_zeroed(L * qa1));
  AQ_TRY(fb->sdam2.alloc_zeroed(L * qa1));
  AQ_TRY(fb->n_iter.alloc_zeroed(qa1));
  AQ_TRY(fb->conv.alloc_zeroed(qa1));
  fb->max_iter = pm.max_iter;
  AQ_TRY(aq_cis_upload(&fb->trace, std::vector<double>((size_t)pm.max_iter * q, std::numeric_limits<double>::quiet_NaN())));
  const size_t blocks = (size_t)(fb->pl.band_bytes / 8), traits = (size_t)(fb->pl.fit_bytes / 8) / (L + 2);   // of the largest batch
  AQ_TRY(fb->Z.alloc(blocks > 0 ? blocks : 1));
  AQ_TRY(fb->A.alloc(blocks > 0 ? L * blocks : 1));
  AQ_TRY(fb->M.alloc(blocks > 0 ? L * blocks : 1));
  AQ_TRY(fb->R.alloc(traits > 0 ? traits : 1));
  AQ_TRY(fb->Rf.alloc(traits > 0 ? traits : 1));
  AQ_TRY(fb->fit.alloc(traits > 0 ? L * traits : 1));
  AQ_TRY(fb->act_items.alloc(blocks > 0 ? blocks / AQ_FM_BLOCK : 1));
  AQ_TRY(fb->act_tiles.alloc(fb->pl.batch_tiles > 0 ? (size_t)fb->pl.batch_tiles : 1));
  AQ_TRY(fb->n_rows.alloc_zeroed(1));
  if (cap > 0) {
    AQ_TRY(fb->row_snp.alloc((size_t)cap));
    AQ_TRY(fb->row_trait.alloc((size_t)cap));
    AQ_TRY(fb->row_effect.alloc((size_t)cap));
    AQ_TRY(fb->row_alpha.alloc((size_t)cap));
    AQ_TRY(fb->row_mu.alloc((size_t)cap));
    AQ_TRY(fb->row_mu2.alloc((size_t)cap));
  }
  return AQ_OK;
}

// one batch: the tiles [k0, k1), their work items [w0, w1) and ordered traits [j0, j0 + qb)
struct AqFmBatch {
  int k0, k1, w0, w1, j0, qb;
};

static AqFmBatch aq_fm_batch(const AqFmBuf &fb, int bi) {
  const aq_cis_work &wk = fb.b.wk;
  AqFmBatch bt{};
  bt.k0 = bi * fb.pl.batch_tiles;
  bt.k1 = std::min(fb.pl.cis.trait_tiles, bt.k0 + fb.pl.batch_tiles);
  bt.w0 = wk.first_item[(size_t)bt.k0];
  bt.w1 = wk.first_item[(size_t)bt.k1];
  bt.j0 = AQ_CIS_TILE * bt.k0;
  bt.qb = std::min(wk.q_active, AQ_CIS_TILE * bt.k1) - bt.j0;
  return bt;
}

static aq_fm_args aq_fm_kernel_args(aq_prep *h, AqFmBuf &fb, const AqFmBatch &bt, const aq_finemap_params &pm, int64_t cap) {
  AqCisBuf &b = fb.b;
  aq_fm_args a{};
  a.Xs = h->Xs.get(); a.Yc = h->Yc.get(); a.d = b.sxx.get();
  a.n = h->n; a.p1 = h->p_kept; a.q = h->q; a.qa = b.wk.q_active; a.L = pm.L;
  a.item_tile = b.item_tile.get(); a.item_p0 = b.item_p0.get(); a.first_item = b.first_item.get();
  a.lo = b.lo.get(); a.hi = b.hi.get(); a.orig = b.order.get();
  a.k0 = bt.k0; a.w0 = bt.w0; a.j0 = bt.j0; a.qb = bt.qb;
  a.act_items = fb.act_items.get(); a.act_tiles = fb.act_tiles.get();
  a.Z = fb.Z.get(); a.A = fb.A.get(); a.M = fb.M.get();
  a.lstride = (size_t)(bt.w1 - bt.w0) * AQ_FM_BLOCK;
  a.R = fb.R.get(); a.Rf = fb.Rf.get(); a.fit = fb.fit.get();
  a.act = fb.act.get(); a.P = fb.P.get(); a.thr = fb.thr.get();
  a.sig2 = fb.sig2.get(); a.sig2_used = fb.sig2_used.get(); a.elbo_prev = fb.elbo_prev.get();
  a.V = fb.V.get(); a.V_used = fb.V_used.get(); a.lbf = fb.lbf.get(); a.szam = fb.szam.get(); a.sdam2 = fb.sdam2.get();
  a.n_iter = fb.n_iter.get(); a.conv = fb.conv.get();
  a.trace = fb.trace.get();
  a.it = 0; a.tol = pm.tol;
  a.row_snp = fb.row_snp.get(); a.row_trait = fb.row_trait.get(); a.row_effect = fb.row_effect.get();
  a.row_alpha = fb.row_alpha.get(); a.row_mu = fb.row_mu.get(); a.row_mu2 = fb.row_mu2.get();
  a.cap = (long long)cap; a.n_rows = fb.n_rows.get();
  return a;
}

// the start of a batch: alpha, mu and the fits 0.0, R = Rf = y in the order.  Asynchronous.
static int aq_fm_batch_start(aq_prep *h, AqFmBuf &fb, const AqFmBatch &bt, const aq_fm_args &a) {
  const size_t qbn = (size_t)bt.qb * (size_t)h->n;
  AQ_HIP(hipMemsetAsync(fb.A.get(), 0, (size_t)a.L * a.lstride * sizeof(double), 0));
  AQ_HIP(hipMemsetAsync(fb.M.get(), 0, (size_t)a.L * a.lstride * sizeof(double), 0));
  AQ_HIP(hipMemsetAsync(fb.fit.get(), 0, (size_t)a.L * qbn * sizeof(double), 0));
  hipLaunchKernelGGL(aq_k_ms_gather, dim3((unsigned)(bt.qb < (1 << 20) ? bt.qb : (1 << 20))), dim3(256), 0, 0, h->Yc.get(),
                     (const int32_t *)(fb.b.order.get() + bt.j0), (const int32_t *)nullptr, h->n, bt.qb, 1, fb.R.get());
  AQ_HIP(hipGetLastError());
  AQ_HIP(hipMemcpyAsync(fb.Rf.get(), fb.R.get(), qbn * sizeof(double), hipMemcpyDeviceToDevice, 0));
  return AQ_OK;
}

// the tiles of the batch with an active trait and their work items, uploaded; *n_items, *n_tiles: how many
static int aq_fm_active_lists(AqFmBuf &fb, const AqFmBatch &bt, unsigned *n_items, unsigned *n_tiles) {
  const aq_cis_work &wk = fb.b.wk;
  std::vector<int32_t> items, tiles;
  for (int k = bt.k0; k < bt.k1; k++) {
    bool any = false;
    for (int j = AQ_CIS_TILE * k; j < AQ_CIS_TILE * (k + 1) && j < wk.q_active; j++) any = any || fb.act_host[(size_t)j] != 0;
    if (!any) continue;
    tiles.push_back(k);
    for (int w = wk.first_item[(size_t)k]; w < wk.first_item[(size_t)k + 1]; w++) items.push_back(w);
  }
  if (!items.empty()) AQ_HIP(hipMemcpy(fb.act_items.get(), items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  if (!tiles.empty()) AQ_HIP(hipMemcpy(fb.act_tiles.get(), tiles.data(), tiles.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  *n_items = (unsigned)items.size();
  *n_tiles = (unsigned)tiles.size();
  return AQ_OK;
}

static void aq_fm_launch_xtr(unsigned n_items, const aq_fm_args &a) {
  aq_screen_a16(a.n, [&](auto a16) { hipLaunchKernelGGL((aq_k_fm_xtr<decltype(a16)::value>), dim3(n_items), dim3(256), 0, 0, a); });
}
static void aq_fm_launch_ser(const aq_fm_args &a, int l) { hipLaunchKernelGGL(aq_k_fm_ser, dim3((unsigned)a.qb), dim3(256), 0, 0, a, l); }
static void aq_fm_launch_fit(unsigned n_tiles, const aq_fm_args &a, int l) {
  hipLaunchKernelGGL(aq_k_fm_fit, dim3(n_tiles, (unsigned)((a.n + AQ_FM_SAMPLE_BLOCK - 1) / AQ_FM_SAMPLE_BLOCK)), dim3(256), 0, 0, a, l);
}
static void aq_fm_launch_iter_end(const aq_fm_args &a) { hipLaunchKernelGGL(aq_k_fm_iter_end, dim3((unsigned)a.qb), dim3(256), 0, 0, a); }

// IBSS of one batch: per iteration the three kernels per effect and the one that ends it, then the active flags back, from
// which the lists of the next iteration are made
static int aq_fm_run_batch(aq_prep *h, AqFmBuf &fb, const AqFmBatch &bt, aq_fm_args a) {
  AQ_TRY(aq_fm_batch_start(h, fb, bt, a));
  for (int it = 0; it < fb.max_iter; it++) {
    unsigned n_items = 0, n_tiles = 0;
    AQ_TRY(aq_fm_active_lists(fb, bt, &n_items, &n_tiles));
    if (n_tiles == 0) break;
    a.it = it;
    for (int l = 0; l < a.L; l++) {
      aq_fm_launch_xtr(n_items, a);
      aq_fm_launch_ser(a, l);
      aq_fm_launch_fit(n_tiles, a, l);
    }
    aq_fm_launch_iter_end(a);
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipMemcpy(fb.act_host.data() + bt.j0, fb.act.get() + bt.j0, (size_t)bt.qb * sizeof(int), hipMemcpyDeviceToHost));
  }
  return AQ_OK;
}

template <typename T>
static int aq_fm_download(std::vector<T> *dst, const AqDev<T> &src, size_t count) {
  dst->resize(count > 0 ? count : 1);
  if (count > 0) AQ_HIP(hipMemcpy(dst->data(), src.get(), count * sizeof(T), hipMemcpyDeviceToHost));
  return AQ_OK;
}

extern "C" int aq_prep_cis_finemap(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, const int32_t *active,
                                   const aq_finemap_params *params, int64_t cap, int32_t *row_snp, int32_t *row_trait, int32_t *row_effect,
                                   double *row_alpha, double *row_mu, double *row_mu2, int64_t *n_rows, double *sigma2, double *V,
                                   double *lbf, double *elbo_trace, int32_t *n_iter, int32_t *converged, int64_t *n_undef,
                                   double *alpha_dense, double *mu_dense, aq_finemap_plan *plan_out) {
  const char *who = "aq_prep_cis_finemap";
  if (!s_lo || !s_hi) return aq_fail(AQ_ERR_ARG, std::string(who) + ": NULL s_lo or s_hi");
  AQ_TRY(aq_fm_check_params(params, who));
  if (cap < 0) return aq_fail(AQ_ERR_ARG, std::string(who) + ": cap >= 0 required, " + std::to_string(cap) + " given");
  if (!h) return aq_fail(AQ_ERR_ARG, std::string(who) + ": NULL handle");
  AQ_TRY(aq_cis_need_windows(h, s_lo, s_hi, who));
  if (h->n < 2) return aq_fail(AQ_ERR_ARG, std::string(who) + ": n >= 2 required");
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout(who));
  const aq_finemap_params pm = *params;
  AqFmBuf fb;
  AQ_TRY(aq_fm_setup(h, s_lo, s_hi, active, pm, cap, who, &fb));
  if (plan_out) *plan_out = fb.pl;
  const aq_cis_work &wk = fb.b.wk;
  const size_t q = (size_t)h->q, qa = (size_t)wk.q_active, p1 = (size_t)h->p_kept, L = (size_t)pm.L;
  const std::vector<int> fitted = fb.act_host;           // per ordered trait: IBSS runs for it
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // what a trait that was asked for gets when IBSS does not run for it: no window, or no predictor with prior weight
  for (size_t t = 0; t < q; t++) {
    if (active && active[t] == 0) continue;
    if (sigma2) sigma2[t] = nan;
    if (n_iter) n_iter[t] = 0;
    if (converged) converged[t] = 0;
    if (n_undef) n_undef[t] = (int64_t)s_hi[t] - (int64_t)s_lo[t];   // less the predictors with weight, below
    for (size_t l = 0; l < L; l++) {
      if (V) V[t * L + l] = nan;
      if (lbf) lbf[t * L + l] = nan;
    }
    if (elbo_trace)
      for (int it = 0; it < pm.max_iter; it++) elbo_trace[(size_t)it * q + t] = nan;
    if (alpha_dense) std::fill(alpha_dense + t * L * p1, alpha_dense + (t + 1) * L * p1, 0.0);
    if (mu_dense) std::fill(mu_dense + t * L * p1, mu_dense + (t + 1) * L * p1, 0.0);
  }
  std::vector<double> hA, hM;
  for (int bi = 0; bi < fb.pl.n_batches; bi++) {
    const AqFmBatch bt = aq_fm_batch(fb, bi);
    const aq_fm_args a = aq_fm_kernel_args(h, fb, bt, pm, cap);
    AQ_TRY(aq_fm_run_batch(h, fb, bt, a));
    hipLaunchKernelGGL(aq_k_fm_rows, dim3((unsigned)(bt.w1 - bt.w0), (unsigned)pm.L), dim3(256), 0, 0, a);
    AQ_HIP(hipGetLastError());
    if (alpha_dense || mu_dense) {                       // tests and small problems: the state of the batch through the host
      const size_t cnt = L * a.lstride;
      AQ_TRY(aq_fm_download(&hA, fb.A, cnt));
      AQ_TRY(aq_fm_download(&hM, fb.M, cnt));
      for (int j = bt.j0; j < bt.j0 + bt.qb; j++) {
        if (!fitted[(size_t)j]) continue;
        const size_t t = (size_t)wk.order[(size_t)j];
        const int kt = j / AQ_CIS_TILE, tl = j % AQ_CIS_TILE, w_first = wk.first_item[(size_t)kt], tile_lo = wk.tile_lo[(size_t)kt];
        for (size_t l = 0; l < L; l++)
          for (int s = s_lo[t]; s < s_hi[t]; s++) {
            const int rel = s - tile_lo;
            const size_t o = l * a.lstride + (size_t)(w_first - bt.w0 + rel / AQ_CIS_TILE) * AQ_FM_BLOCK +
                             (size_t)(tl * AQ_CIS_TILE + rel % AQ_CIS_TILE);
            if (alpha_dense) alpha_dense[(t * L + l) * p1 + (size_t)s] = hA[o];
            if (mu_dense) mu_dense[(t * L + l) * p1 + (size_t)s] = hM[o];
          }
      }
    }
    AQ_HIP(hipDeviceSynchronize());                      // the next batch overwrites the state
  }
  unsigned long long cnt = 0;
  AQ_HIP(hipMemcpy(&cnt, fb.n_rows.get(), sizeof(cnt), hipMemcpyDeviceToHost));
  if (n_rows) *n_rows = (int64_t)cnt;
  const size_t rows = cnt < (unsigned long long)cap ? (size_t)cnt : (size_t)cap;
  if (rows > 0) {
    if (row_snp) AQ_HIP(hipMemcpy(row_snp, fb.row_snp.get(), rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (row_trait) AQ_HIP(hipMemcpy(row_trait, fb.row_trait.get(), rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (row_effect) AQ_HIP(hipMemcpy(row_effect, fb.row_effect.get(), rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (row_alpha) AQ_HIP(hipMemcpy(row_alpha, fb.row_alpha.get(), rows * sizeof(double), hipMemcpyDeviceToHost));
    if (row_mu) AQ_HIP(hipMemcpy(row_mu, fb.row_mu.get(), rows * sizeof(double), hipMemcpyDeviceToHost));
    if (row_mu2) AQ_HIP(hipMemcpy(row_mu2, fb.row_mu2.get(), rows * sizeof(double), hipMemcpyDeviceToHost));
  }
  std::vector<double> hs2, hV, hlbf, htrace;
  std::vector<int32_t> hit, hconv;
  AQ_TRY(aq_fm_download(&hs2, fb.sig2, qa));
  AQ_TRY(aq_fm_download(&hV, fb.V, L * qa));
  AQ_TRY(aq_fm_download(&hlbf, fb.lbf, L * qa));
  AQ_TRY(aq_fm_download(&hit, fb.n_iter, qa));
  AQ_TRY(aq_fm_download(&hconv, fb.conv, qa));
  if (elbo_trace) AQ_TRY(aq_fm_download(&htrace, fb.trace, (size_t)pm.max_iter * q));
  for (size_t j = 0; j < qa; j++) {
    const size_t t = (size_t)wk.order[j];
    if (active && active[t] == 0) continue;
    if (n_undef) n_undef[t] -= fb.P_host[j];
    if (!fitted[j]) continue;
    if (sigma2) sigma2[t] = hs2[j];
    if (n_iter) n_iter[t] = hit[j];
    if (converged) converged[t] = hconv[j];
    for (size_t l = 0; l < L; l++) {
      if (V) V[t * L + l] = hV[l * qa + j];
      if (lbf) lbf[t * L + l] = hlbf[l * qa + j];
    }
    if (elbo_trace)
      for (int it = 0; it < pm.max_iter; it++) elbo_trace[(size_t)it * q + t] = htrace[(size_t)it * q + t];
  }
  return AQ_OK;
}

extern "C" int aq_prep_set_purity(aq_prep_handle h, const int32_t *set_ptr, const int32_t *set_idx, int32_t n_sets, double *min_abs_r,
                                  double *mean_abs_r) {
  const std::string w("aq_prep_set_purity");
  if (!set_ptr || !set_idx || !min_abs_r || !mean_abs_r) return aq_fail(AQ_ERR_ARG, w + ": NULL argument");
  if (n_sets < 0) return aq_fail(AQ_ERR_ARG, w + ": n_sets >= 0 required");
  if (!h) return aq_fail(AQ_ERR_ARG, w + ": NULL handle");
  if (set_ptr[0] != 0) return aq_fail(AQ_ERR_ARG, w + ": set_ptr[0] must be 0");
  for (int b = 0; b < n_sets; b++) {
    const long long m = (long long)set_ptr[b + 1] - set_ptr[b];
    if (m < 1 || m > AQ_FM_PURITY_MAX)
      return aq_fail(AQ_ERR_ARG, w + ": set " + std::to_string(b) + " has " + std::to_string(m) + " members; 1 ... " +
                                     std::to_string(AQ_FM_PURITY_MAX) + " are supported");
    for (int e = set_ptr[b]; e < set_ptr[b + 1]; e++)
      if (set_idx[e] < 0 || set_idx[e] >= h->p_kept)
        return aq_fail(AQ_ERR_ARG, w + ": set " + std::to_string(b) + " names the column " + std::to_string(set_idx[e]) + " outside [0, " +
                                       std::to_string(h->p_kept) + ")");
  }
  if (n_sets == 0) return AQ_OK;
  AQ_TRY(aq_need_device(h->device));
  AqDev<int32_t> dptr, didx;
  AqDev<double> dmin, dmean;
  AQ_TRY(aq_cis_upload(&dptr, std::vector<int32_t>(set_ptr, set_ptr + n_sets + 1)));
  AQ_TRY(aq_cis_upload(&didx, std::vector<int32_t>(set_idx, set_idx + set_ptr[n_sets])));
  AQ_TRY(dmin.alloc((size_t)n_sets));
  AQ_TRY(dmean.alloc((size_t)n_sets));
  hipLaunchKernelGGL(aq_k_fm_purity, dim3((unsigned)n_sets), dim3(256), 0, 0, h->Xs.get(), h->n, dptr.get(), didx.get(), dmin.get(),
                     dmean.get());
  AQ_HIP(hipGetLastError());
  AQ_HIP(hipMemcpy(min_abs_r, dmin.get(), (size_t)n_sets * sizeof(double), hipMemcpyDeviceToHost));
  AQ_HIP(hipMemcpy(mean_abs_r, dmean.get(), (size_t)n_sets * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}

// Timing hook: the four kernels of one IBSS iteration with the default parameters, every batch from its start, all traits
// active.  Per batch each kernel is timed on its own, `reps` times between two events after a warm-up, on effect 0 (a launch
// costs the same for every effect); an iteration launches the first three L times, so ms_xtr, ms_ser and ms_fit are L times the
// launch, summed over the batches, and ms_iter_end is the one launch, summed.
extern "C" int aq_prep_cis_finemap_time(aq_prep_handle h, const int32_t *s_lo, const int32_t *s_hi, int32_t L, int32_t reps, double *ms_xtr,
                                        double *ms_ser, double *ms_fit, double *ms_iter_end, aq_finemap_plan *plan_out) {
  const char *who = "aq_prep_cis_finemap_time";
  if (!s_lo || !s_hi || !ms_xtr || !ms_ser || !ms_fit || !ms_iter_end) return aq_fail(AQ_ERR_ARG, std::string(who) + ": NULL argument");
  if (reps < 1) return aq_fail(AQ_ERR_ARG, std::string(who) + ": reps >= 1 required");
  aq_finemap_params pm{};
  pm.L = L; pm.max_iter = 1; pm.tol = 0.0; pm.scaled_prior_variance = 0.2; pm.coverage = 0.95; pm.alpha_min = 1e-4;
  AQ_TRY(aq_fm_check_params(&pm, who));
  if (!h) return aq_fail(AQ_ERR_ARG, std::string(who) + ": NULL handle");
  AQ_TRY(aq_cis_need_windows(h, s_lo, s_hi, who));
  if (h->n < 2) return aq_fail(AQ_ERR_ARG, std::string(who) + ": n >= 2 required");
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout(who));
  AqFmBuf fb;
  AQ_TRY(aq_fm_setup(h, s_lo, s_hi, nullptr, pm, 0, who, &fb));
  if (plan_out) *plan_out = fb.pl;
  *ms_xtr = *ms_ser = *ms_fit = *ms_iter_end = 0.0;
  for (int bi = 0; bi < fb.pl.n_batches; bi++) {
    const AqFmBatch bt = aq_fm_batch(fb, bi);
    const aq_fm_args a = aq_fm_kernel_args(h, fb, bt, pm, 0);
    AQ_TRY(aq_fm_batch_start(h, fb, bt, a));
    unsigned n_items = 0, n_tiles = 0;
    AQ_TRY(aq_fm_active_lists(fb, bt, &n_items, &n_tiles));
    if (n_tiles == 0) continue;
    double ms = 0.0;
    const auto timed = [&](double *sum, double times, auto launch) {
      AQ_TRY(aq_time_launches(reps, &ms, [&] {
        launch();
        AQ_HIP(hipGetLastError());
        return (int)AQ_OK;
      }));
      *sum += times * ms;
      return (int)AQ_OK;
    };
    AQ_TRY(timed(ms_xtr, (double)L, [&] { aq_fm_launch_xtr(n_items, a); }));
    AQ_TRY(timed(ms_ser, (double)L, [&] { aq_fm_launch_ser(a, 0); }));
    AQ_TRY(timed(ms_fit, (double)L, [&] { aq_fm_launch_fit(n_tiles, a, 0); }));
    AQ_TRY(timed(ms_iter_end, 1.0, [&] { aq_fm_launch_iter_end(a); }));
  }
  return AQ_OK;
}
