// aq_vb_create.hip -- aq_vb_create: validation, the one pass over Y for missing values, the launch plan, allocation, upload and
// layout conversion, the initial loop state; and aq_vb_destroy.  The handle owns every device buffer it allocates (aq_vb.h), so
// every error path below simply returns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "aq_vb.h"
#include "aq_setup_kernels.h"

static int aq_upload_padded(double *dst, const double *src, size_t n, size_t n_pad) {
  AQ_HIP(hipMemset(dst, 0, n_pad * sizeof(double)));
  AQ_HIP(hipMemcpy(dst, src, n * sizeof(double), hipMemcpyHostToDevice));
  return AQ_OK;
}

// Environment overrides of the launch plan (test and experiment hooks: AQ_TT, AQ_CHAIN, AQ_LA_C, ...).  Every one the planner
// finds SET when a handle is created is recorded in the handle and reported by aq_vb_get_overrides, so that a host which
// inherits such a variable from its environment -- an R session, a batch script -- can see that the plan is not the library's own.
static AqEnv aq_env_recorder(std::string *found) {
  return [found](const char *name) {
    const char *v = getenv(name);
    if (v) *found += (found->empty() ? "" : " ") + std::string(name) + "=" + v;
    return v;
  };
}

extern "C" int64_t aq_vb_reduce_len(int32_t p) { return (int64_t)((p + 15) / 16) * 16 + AQ_RED_EXTRA; }

// get_annealing_ladder_, R/utils.R:108-146
static std::vector<double> aq_ladder(const double anneal[3]) {
  double k_m = 1.0 / anneal[1];
  int m = (int)std::llround(anneal[2]);
  std::vector<double> l(m);
  int type = (int)std::llround(anneal[0]);
  if (type == 1) {
    double delta = std::pow(k_m, 1.0 / (1 - m)) - 1;
    for (int i = 0; i < m; i++) l[i] = std::pow(1 + delta, 1.0 - (double)(m - i));
  } else if (type == 2) {
    double delta = (1 / k_m - 1) / (m - 1);
    for (int i = 0; i < m; i++) l[i] = 1.0 / (1 + delta * ((double)(m - i) - 1));
  } else {
    double delta = (1 - k_m) / (m - 1);
    for (int i = 0; i < m; i++) l[i] = k_m + delta * (double)i;
  }
  return l;
}


// The argument blocks of the kernels, filled once from the buffers and sizes that are fixed from here on.  The launchers of
// aq_vb_sweep.hip set only what varies per launch.  XR is null by now for the MASK instances of the look-ahead kernel (released
// once the GK blocks are built) and live for the masked two-barrier kernel.
static void aq_fill_args(aq_vb *s) {
  AqCoreArgs &a = s->core_args;
  a.XA = s->XA.get(); a.XU = s->XU.get(); a.G = s->G.get(); a.Gx = s->Gx.get(); a.R = s->R.get(); a.gam = s->gam.get(); a.mu = s->mu.get();
  a.theta = s->theta.get(); a.zeta = s->zeta.get();
  a.Aarr = s->Aarr.get(); a.Barr = s->Barr.get(); a.coef = s->coef.get(); a.inv2s = s->inv2s.get(); a.cst = s->cst.get(); a.sig2b = s->sig2b.get();
  a.sums = s->sums.get(); a.rowGB = s->rowGB.get();
  a.p = s->p; a.q = s->q; a.p_pad = s->p_pad; a.q_pad = s->q_pad; a.n_pad = s->n_pad; a.nb = s->nb; a.ntile = s->ntile;
  a.dmode = s->dmode;
  a.done = s->done.get(); a.errflag = s->errflag.get(); a.stagger = s->stagger;
  a.C = s->laC; a.xhelper = s->la_xhelper; a.Pbuf = s->Pbuf.get(); a.pflag = s->pflag.get(); a.rnpart = s->rnpart.get();
  a.xtouch = s->la_xtouch;
  a.hprio = s->la_hprio;
  a.mprio = s->la_mprio;
  a.mis = s->mis.get(); a.GK = s->GK.get(); a.tau = s->tau.get(); a.log_tau = s->log_tau.get();
  a.sig2_inv_p = &s->sc.get()->sig2_inv; a.log_sig2_inv_p = &s->sc.get()->log_sig2_inv;

  AqMisArgs &m = s->mis_args;
  m.XA = s->XA.get(); m.XU = s->XU.get(); m.G = s->G.get(); m.XR = s->XR.get(); m.R = s->R.get(); m.mis = s->mis.get(); m.gam = s->gam.get(); m.mu = s->mu.get();
  m.Aarr = s->Aarr.get(); m.Barr = s->Barr.get(); m.tau = s->tau.get(); m.log_tau = s->log_tau.get(); m.sig2b = s->sig2b.get(); m.sc = s->sc.get();
  m.midx = s->midx.get(); m.mcnt4 = s->mcnt4.get(); m.sums = s->sums.get(); m.rowGB = s->rowGB.get();
  m.p = s->p; m.q = s->q; m.p_pad = s->p_pad; m.q_pad = s->q_pad; m.n_pad = s->n_pad; m.nb = s->nb; m.ntile = s->ntile;
  m.dmode = s->dmode; m.NR = s->NR; m.Mmax = s->Mmax;
  m.C = s->misC; m.Pbuf = s->Pbuf.get(); m.pflag = s->pflag.get(); m.errflag = s->errflag.get(); m.rnpart = s->rnpart.get();
  m.done = s->done.get();

  AqTwArgs &t = s->tw_args;
  t.X = s->Xcm.get(); t.R = s->R.get(); t.mis = s->mis.get(); t.XN = s->XN.get(); t.gam = s->gam.get(); t.mu = s->mu.get(); t.Aarr = s->Aarr.get(); t.Barr = s->Barr.get();
  t.tau = s->tau.get(); t.log_tau = s->log_tau.get(); t.sig2b = s->sig2b.get(); t.sc = s->sc.get(); t.sums = s->sums.get(); t.rowGB = s->rowGB.get();
  t.n = s->n; t.p = s->p; t.q = s->q; t.n_pad = s->n_pad; t.p_pad = s->p_pad; t.q_pad = s->q_pad; t.ntile = s->ntile;
  t.complete = s->has_missing ? 0 : 1;
  t.ns = s->tw_ns;

  AqPrepass &v = s->pre_args;
  v.theta = s->theta.get(); v.zeta = s->zeta.get(); v.gam = s->gam.get(); v.Aarr = s->Aarr.get(); v.Barr = s->Barr.get(); v.rowA = s->rowA.get();
  v.colApart = s->colApart.get(); v.Hpart = s->Hpart.get(); v.p = s->p; v.q = s->q; v.p_pad = s->p_pad; v.q_pad = s->q_pad;
  v.rows_per_chunk = s->rows_per_chunk;
  v.write_AB = s->fused ? 0 : 1;

  AqQvec &qv = s->qv;
  qv.eta_h = s->eta_h.get(); qv.kappa_h = s->kappa_h.get(); qv.n0 = s->n0.get(); qv.nobs = s->nobs.get();
  qv.zeta = s->zeta.get(); qv.tau = s->tau.get(); qv.sig2b = s->sig2b.get(); qv.log_tau = s->log_tau.get(); qv.eta_vb = s->eta_vb.get();
  qv.kappa_vb = s->kappa_vb.get(); qv.coef = s->coef.get(); qv.inv2s = s->inv2s.get(); qv.cst = s->cst.get(); qv.sums = s->sums.get();
  qv.colApart = s->colApart.get(); qv.nchunk = s->fused ? 0 : s->nHchunk;   // fused: colSums(a) is already inside sums[3]
  qv.q = s->q; qv.q_pad = s->q_pad; qv.n = s->n; qv.nu_h = s->nu; qv.rho_h = s->rho;
  qv.na = s->has_missing ? 1 : 0;

  AqPvec &pv = s->pv;
  pv.theta = s->theta.get(); pv.sig2_theta = s->sig2_theta.get(); pv.L = s->L.get(); pv.lam2_inv = s->lam2_inv.get(); pv.Q = s->Q.get();
  pv.rsZ = s->red; pv.part = s->ppart.get(); pv.p = s->p; pv.p_pad = s->p_pad; pv.shr = s->shr; pv.m0 = s->m0;
  pv.A2_inv = s->A2_inv; pv.df = (double)s->df;
}

extern "C" int aq_vb_create(const aq_vb_problem *pr, aq_vb_handle *out) {
  if (!pr || !out) return aq_fail(AQ_ERR_ARG, "aq_vb_create: NULL argument");
  *out = nullptr;
  if (pr->n < 2 || pr->p < 1 || pr->q < 1) return aq_fail(AQ_ERR_ARG, "aq_vb_create: n >= 2, p >= 1, q >= 1 required");
  if (pr->q_total < pr->q) return aq_fail(AQ_ERR_ARG, "aq_vb_create: q_total < q");
  if (!pr->X || !pr->Y || !pr->eta || !pr->kappa || !pr->n0 || (!pr->init_generate && (!pr->gam_vb || !pr->mu_beta_vb)) || !pr->sig2_beta_vb ||
      !pr->sig2_theta_vb || !pr->tau_vb || !pr->theta_vb || !pr->zeta_vb)
    return aq_fail(AQ_ERR_ARG, "aq_vb_create: NULL data pointer");
  if (!(pr->tol > 0)) return aq_fail(AQ_ERR_ARG, "tol must be positive");
  if (pr->maxit < 1) return aq_fail(AQ_ERR_ARG, "maxit must be natural.");
  if (pr->has_anneal) {   // check_annealing_, R/prepare_atlasqtl.R:100-124
    int type = (int)std::llround(pr->anneal[0]);
    if (type < 1 || type > 3)
      return aq_fail(AQ_ERR_ARG, "The annealing spacing scheme must be set to 1 for geometric 2 for harmonic or 3 for linear spacing.");
    if (pr->anneal[1] < 1.5) return aq_fail(AQ_ERR_ARG, "Initial annealing temperature very small.");
    if (pr->anneal[2] > 1000 || pr->anneal[2] < 2) return aq_fail(AQ_ERR_ARG, "Temperature grid size out of range.");
  }
  if (pr->world_size < 1) return aq_fail(AQ_ERR_ARG, "world_size must be >= 1");
  if (pr->scheme != 0 && pr->scheme != 1) return aq_fail(AQ_ERR_ARG, "scheme must be 0 (global-local horseshoe) or 1 (global-only)");
  const int df = pr->df == 0 ? 1 : pr->df;
  if (pr->scheme == 0 && df != 1 && df != 3 && df != 5 && df != 7)
    return aq_fail(AQ_ERR_UNSUPPORTED, "df must be 1, 3, 5 or 7 (the reference calls compute_integral_hs_ unstable from df = 9 on, R/utils.R:510)");
  AQ_TRY(aq_need_device(pr->device));

  // X must be complete; Y may hold NaN.  With xy_on_device both are device pointers: X is trusted to be the standardised
  // NaN-free matrix of aq_prepare_data, Y (n x q, small) is copied back once for the missingness bookkeeping below.
  size_t np = (size_t)pr->n * pr->p, nq = (size_t)pr->n * pr->q;
  std::vector<double> Yhost;
  const double *Yh = pr->Y;
  const bool x_dev = (pr->xy_on_device & 1) != 0, y_dev = (pr->xy_on_device & 2) != 0;
  if (y_dev) {
    Yhost.resize(nq);
    AQ_HIP(hipMemcpy(Yhost.data(), pr->Y, nq * sizeof(double), hipMemcpyDeviceToHost));
    Yh = Yhost.data();
  }
  if (!x_dev) {
    for (size_t i = 0; i < np; i++)
      if (!(pr->X[i] == pr->X[i])) return aq_fail(AQ_ERR_ARG, "X must be a non-empty a numeric matrix, finite without missing value.");
  }
  // the one pass over Y for missing values: per trait the count, from which the planner's inputs, nobs and the index lists derive
  std::vector<int> nmiss(pr->q, 0);
  AqPlanInput in;
  in.n = pr->n; in.p = pr->p; in.q = pr->q;
  for (int k = 0; k < pr->q; k++) {
    const double *yk = Yh + (size_t)pr->n * k;
    int m = 0;
    for (int i = 0; i < pr->n; i++) m += !(yk[i] == yk[i]);
    nmiss[k] = m;
    in.max_missing = std::max(in.max_missing, m);
    in.max_short_list = std::max(in.max_short_list, std::min(m, pr->n - m));
  }
  in.has_missing = in.max_missing > 0;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, pr->device) == hipSuccess && prop.multiProcessorCount > 0) in.ncu = prop.multiProcessorCount;
    size_t free_b = 0, tot_b = 0;
    const hipError_t mrc = hipMemGetInfo(&free_b, &tot_b);
    if (mrc == hipSuccess) in.total_bytes = (long long)tot_b;
    else in.mem_error = hipGetErrorString(mrc);
  }
  std::string overrides;
  AqPlan plan;
  {
    std::string err;
    const int rc = aq_make_plan(in, aq_env_recorder(&overrides), &plan, &err);
    if (rc != AQ_OK) return aq_fail(rc, err);
  }
  int dmode = 0;
  AQ_TRY(aq_probe_dmode(&dmode));
  if ((plan.use_la || plan.use_mis) && dmode != 0)   // the MFMA sweep kernels are written for gfx950's accumulator map (row = 4 reg + lane / 16)
    return aq_fail(AQ_ERR_UNSUPPORTED, "this device reports an f64 MFMA accumulator layout the sweep kernels are not written for");


  std::unique_ptr<aq_vb> s(new aq_vb());   // owns every buffer allocated below until it is handed to the caller
  static_cast<AqPlan &>(*s) = plan;
  s->overrides = overrides;
  s->dmode = dmode;
  s->device = pr->device;
  s->n = pr->n; s->p = pr->p; s->q = pr->q; s->q_total = pr->q_total; s->world = pr->world_size;
  s->trait_offset = pr->trait_offset;
  s->A2_inv = pr->A2_inv; s->m0 = pr->m0; s->nu = pr->nu; s->rho = pr->rho; s->t02 = pr->t02;
  s->t02_inv = 1.0 / pr->t02;
  s->shr = (double)pr->q_total;   // shr_fac_inv <- q, R/atlasqtl.R:218
  s->has_anneal = pr->has_anneal != 0;
  s->scheme = pr->scheme; s->df = pr->scheme == 1 ? 1 : (pr->df == 0 ? 1 : pr->df);
  std::memcpy(s->anneal, pr->anneal, sizeof(s->anneal));
  s->tol = pr->tol; s->maxit = pr->maxit; s->thinned = pr->thinned_elbo_eval != 0; s->debug = pr->debug != 0;
  s->has_missing = in.has_missing || s->use_mis || s->la_mask;   // the masked kernel produces the NA forms of the column sums (identical for complete Y)

  const int NTT = s->n_pad / 16;
  size_t xelems = s->use_tw ? 1 : (size_t)s->nb * NTT * 128;
  AQ_TRY(s->XA.alloc_zeroed(xelems));
  AQ_TRY(s->XU.alloc_zeroed(xelems));
  AQ_TRY(s->G.alloc_zeroed((size_t)s->nb * 256));
  AQ_TRY(s->Gx.alloc_zeroed((size_t)s->nb * 256));
  if (s->use_tw) {
    AQ_TRY(s->mis.alloc_zeroed((size_t)s->ntile * s->n_pad * 16));
    AQ_TRY(s->XN.alloc_zeroed((size_t)s->ntile * s->p_pad * 16));
  }
  if (s->use_mis || s->la_mask) {
    AQ_TRY(s->mis.alloc_zeroed((size_t)s->ntile * s->n_pad * 16));
    AQ_TRY(s->XR.alloc_zeroed((size_t)s->nb * s->NR * 16));
    AQ_TRY(s->midx.alloc_zeroed((size_t)s->ntile * 16 * s->Mmax));
    AQ_TRY(s->mcnt4.alloc_zeroed((size_t)s->ntile * 16));
    if (s->use_mis) {
      AQ_TRY(s->Pbuf.alloc_zeroed(aq_pbuf_elems(*s)));
      AQ_TRY(s->pflag.alloc_zeroed((size_t)s->ntile * s->misC));
      AQ_TRY(s->rnpart.alloc_zeroed((size_t)s->misC * s->q_pad));
    }
    // lists of missing samples per trait, padded to groups of 16 with the all-zero row n_pad of XR
    std::vector<int> idx((size_t)s->ntile * 16 * s->Mmax, s->n_pad), cnt((size_t)s->ntile * 16, 0), obs((size_t)s->ntile * 16, 0);
    for (int k = 0; k < s->q; k++) {
      int m = 0;
      int *dst = idx.data() + (size_t)k * s->Mmax;      // trait k = tile (k / 16), slot (k % 16): contiguous
      const double *yk = Yh + (size_t)s->n * k;
      const bool list_obs = s->la_wide && 2 * nmiss[k] > s->n;   // wide split: more missing than observed -- list the observed samples
      obs[k] = list_obs ? 1 : 0;
      for (int i = 0; i < s->n; i++)
        if ((yk[i] == yk[i]) == list_obs) dst[m++] = i;
      cnt[k] = (m + 15) / 16 * 4;
    }
    if (s->la_wide) {
      AQ_TRY(s->mobs.alloc_zeroed(obs.size()));
      AQ_HIP(hipMemcpy(s->mobs.get(), obs.data(), obs.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    AQ_HIP(hipMemcpy(s->midx.get(), idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
    AQ_HIP(hipMemcpy(s->mcnt4.get(), cnt.data(), cnt.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  if (s->use_la && s->laC > 1) {
    AQ_TRY(s->Pbuf.alloc_zeroed(aq_pbuf_elems(*s)));
    AQ_TRY(s->pflag.alloc_zeroed((size_t)s->ntile * s->laC));
    AQ_TRY(s->rnpart.alloc_zeroed((size_t)s->laC * s->q_pad));
  }
  AQ_TRY(s->R.alloc_zeroed((size_t)s->ntile * s->n_pad * 16));
  AQ_TRY(s->gam.alloc_zeroed((size_t)s->ntile * s->p_pad * 16));
  AQ_TRY(s->mu.alloc_zeroed((size_t)s->ntile * s->p_pad * 16));
  AQ_TRY(s->theta.alloc_zeroed((size_t)s->p_pad));
  AQ_TRY(s->sig2_theta.alloc_zeroed((size_t)s->p_pad));
  AQ_TRY(s->L.alloc_zeroed((size_t)s->p_pad));
  AQ_TRY(s->lam2_inv.alloc_zeroed((size_t)s->p_pad));
  AQ_TRY(s->Q.alloc_zeroed((size_t)s->p_pad));
  s->pblk = (s->p + 255) / 256;
  AQ_TRY(s->ppart.alloc_zeroed((size_t)3 * s->pblk));
  AqDev<double> *qvecs[] = {&s->eta_h, &s->kappa_h, &s->n0, &s->nobs, &s->zeta, &s->tau, &s->sig2b, &s->log_tau, &s->eta_vb,
                            &s->kappa_vb, &s->coef, &s->inv2s, &s->cst};
  for (AqDev<double> *qp : qvecs) AQ_TRY(qp->alloc_zeroed((size_t)s->q_pad));
  AQ_TRY(s->sums.alloc_zeroed((size_t)6 * s->q_pad * (s->chain + 2)));   // one slot of 5 (look-ahead) or 6 (NA forms) rows per chained segment
  AQ_TRY(s->done.alloc_zeroed((size_t)s->ntile));
  AQ_TRY(s->errflag.alloc_zeroed((size_t)1));
  s->fused = s->use_la;   // the look-ahead kernel computes A, b and the sums of a itself: no pre-pass arrays
  if (!s->fused) AQ_TRY(s->rowA.alloc_zeroed((size_t)s->ntile * s->p_pad));
  AQ_TRY(s->rowGB.alloc_zeroed((size_t)s->ntile * s->WPT * s->p_pad));
  if (!s->fused) {   // the other kernels read A and b from the pre-pass arrays
    AQ_TRY(s->Aarr.alloc_zeroed((size_t)s->ntile * s->p_pad * 16));
    AQ_TRY(s->Barr.alloc_zeroed((size_t)s->ntile * s->p_pad * 16));
  }
  if (pr->ext_reduce_main) { s->red = pr->ext_reduce_main; }
  else { AQ_TRY(s->red_own.alloc_zeroed((size_t)aq_vb_reduce_len(s->p))); s->red = s->red_own.get(); }
  if (pr->ext_reduce_elbo) { s->ered = pr->ext_reduce_elbo; }
  else { AQ_TRY(s->ered_own.alloc_zeroed((size_t)8)); s->ered = s->ered_own.get(); }
  s->rows_per_chunk = 2048;
  s->nHchunk = (s->p_pad + s->rows_per_chunk - 1) / s->rows_per_chunk;
  AQ_TRY(s->Hpart.alloc_zeroed((size_t)s->ntile * s->nHchunk));
  AQ_TRY(s->colApart.alloc_zeroed((size_t)s->nHchunk * s->q_pad));
  AQ_TRY(s->sc.alloc_zeroed((size_t)1));

  // ---- uploads + layout conversion (staging buffers freed afterwards) ----
  {
    AqDev<double> Xown;
    const double *Xd = pr->X;
    const bool own_x = !x_dev || s->use_tw;   // the generic kernel keeps X: it needs a copy of its own
    if (own_x) {
      AQ_TRY(Xown.alloc(np));
      AQ_HIP(hipMemcpy(Xown.get(), pr->X, np * sizeof(double), x_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
      Xd = Xown.get();
    }
    if (s->use_tw) {
      s->Xcm = std::move(Xown);   // the generic kernel reads X column-major as given
    } else {
      hipLaunchKernelGGL(aq_k_build_x_layouts, dim3((unsigned)((xelems + 255) / 256)), dim3(256), 0, 0, Xd, s->XA.get(), s->XU.get(),
                         s->n, s->p, s->nb, NTT, s->dmode);
      hipLaunchKernelGGL(aq_k_gram_blocks, dim3(s->nb), dim3(256), 0, 0, Xd, s->G.get(), s->Gx.get(), s->n, s->p);
      if (s->use_mis || s->la_mask) {
        size_t tot = (size_t)s->nb * s->NR * 16;
        hipLaunchKernelGGL(aq_k_build_xr, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0, Xd, s->XR.get(), s->n, s->p, s->nb, s->NR);
      }
      AQ_HIP(hipDeviceSynchronize());
      Xown.reset();
      if (s->la_mask) {
        // the traits' own Gram blocks, once per handle (aq_setup_kernels.h::aq_k_gk_blocks); the row panels are not needed after
        AQ_TRY(s->GK.alloc_zeroed((size_t)s->ntile * s->nb * AQ_GK_STRIDE));
        const int bchunk = 32;
        if (s->la_wide)   // lists of any length, from global memory (aq_setup_kernels.h::aq_k_gk_blocks_g)
          hipLaunchKernelGGL(aq_k_gk_blocks_g, dim3((s->nb + bchunk - 1) / bchunk, s->ntile), dim3(512), 0, 0, s->XR.get(), s->G.get(), s->Gx.get(),
                             s->midx.get(), s->mcnt4.get(), s->mobs.get(), s->GK.get(), s->nb, s->NR, s->Mmax, bchunk);
        else
        hipLaunchKernelGGL(aq_k_gk_blocks, dim3((s->nb + bchunk - 1) / bchunk, s->ntile), dim3(512), aq_midx_lds_bytes(s->Mmax), 0, s->XR.get(),
                           s->G.get(), s->Gx.get(), s->midx.get(), s->mcnt4.get(), s->GK.get(), s->nb, s->NR, s->Mmax, bchunk);
        {   // X_norm_sq(j, k) where that subtraction cancels (aq_setup_kernels.h::aq_k_gk_diag_exact)
          const size_t tot = (size_t)s->ntile * s->nb * 256;
          hipLaunchKernelGGL(aq_k_gk_diag_exact, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0, s->XR.get(), s->G.get(), s->midx.get(),
                             s->mcnt4.get(), s->la_wide ? s->mobs.get() : (const int *)nullptr, s->GK.get(), s->n, s->nb, s->ntile, s->NR,
                             s->Mmax);
        }
        AQ_HIP(hipGetLastError());
        AQ_HIP(hipDeviceSynchronize());
        s->XR.reset();
      }
    }
  }
  {
    size_t big = (pr->init_on_device || pr->init_generate) ? nq : std::max((size_t)pr->p * pr->q, nq);
    AqDev<double> stage;
    AQ_TRY(stage.alloc(big));
    AQ_HIP(hipMemcpy(stage.get(), pr->Y, nq * sizeof(double), y_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    AQ_TRY(aq_tile_from_colmajor(stage.get(), s->R.get(), s->n, s->q, s->n_pad, s->ntile, 1));
    AQ_HIP(hipDeviceSynchronize());
    if (s->use_tw || s->use_mis || s->la_mask) {   // mis_pat <- ifelse(is.na(Y), 0, 1), R/atlasqtl_global_local_core.R:21
      std::vector<double> mk(nq);
      for (size_t i = 0; i < nq; i++) mk[i] = (Yh[i] == Yh[i]) ? 1.0 : 0.0;
      AQ_HIP(hipMemcpy(stage.get(), mk.data(), nq * sizeof(double), hipMemcpyHostToDevice));
      AQ_TRY(aq_tile_from_colmajor(stage.get(), s->mis.get(), s->n, s->q, s->n_pad, s->ntile, 0));
      AQ_HIP(hipDeviceSynchronize());
    }
    size_t pq = (size_t)pr->p * pr->q;
    const double *gsrc = pr->gam_vb, *msrc = pr->mu_beta_vb;
    if (pr->init_generate) {
      if (!(pr->init_gam_sd > 0.0)) return aq_fail(AQ_ERR_ARG, "init_gam_sd must be positive");
      size_t tot = (size_t)s->ntile * s->p_pad * 16;
      hipLaunchKernelGGL(aq_k_init_generate, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0, s->gam.get(), s->mu.get(), s->p, s->q, s->p_pad,
                         s->ntile, (unsigned long long)pr->init_seed, (int)pr->trait_offset, pr->init_gam_mean, pr->init_gam_sd);
      AQ_HIP(hipDeviceSynchronize());
    } else {
    if (!pr->init_on_device) {
      AQ_HIP(hipMemcpy(stage.get(), pr->gam_vb, pq * sizeof(double), hipMemcpyHostToDevice));
      gsrc = stage.get();
    }
    AQ_TRY(aq_tile_from_colmajor(gsrc, s->gam.get(), s->p, s->q, s->p_pad, s->ntile, 0));
    AQ_HIP(hipDeviceSynchronize());
    if (!pr->init_on_device) {
      AQ_HIP(hipMemcpy(stage.get(), pr->mu_beta_vb, pq * sizeof(double), hipMemcpyHostToDevice));
      msrc = stage.get();
    }
    AQ_TRY(aq_tile_from_colmajor(msrc, s->mu.get(), s->p, s->q, s->p_pad, s->ntile, 0));
    AQ_HIP(hipDeviceSynchronize());
    }
  }
  AQ_TRY(aq_upload_padded(s->theta.get(), pr->theta_vb, s->p, s->p_pad));
  AQ_TRY(aq_upload_padded(s->sig2_theta.get(), pr->sig2_theta_vb, s->p, s->p_pad));
  AQ_TRY(aq_upload_padded(s->eta_h.get(), pr->eta, s->q, s->q_pad));
  AQ_TRY(aq_upload_padded(s->kappa_h.get(), pr->kappa, s->q, s->q_pad));
  AQ_TRY(aq_upload_padded(s->n0.get(), pr->n0, s->q, s->q_pad));
  AQ_TRY(aq_upload_padded(s->zeta.get(), pr->zeta_vb, s->q, s->q_pad));
  AQ_TRY(aq_upload_padded(s->tau.get(), pr->tau_vb, s->q, s->q_pad));
  AQ_TRY(aq_upload_padded(s->sig2b.get(), pr->sig2_beta_vb, s->q, s->q_pad));
  {
    std::vector<double> nobs(s->q_pad, 0.0);
    for (int k = 0; k < s->q; k++) nobs[k] = (double)(s->n - nmiss[k]);   // colSums(mis_pat), R/update_vb.R:132
    AQ_HIP(hipMemcpy(s->nobs.get(), nobs.data(), nobs.size() * sizeof(double), hipMemcpyHostToDevice));
    // padded traits need valid constants for the init-mode core kernel (coef/inv2s/cst unused there)
    std::vector<double> ones(s->q_pad, 1.0);
    AQ_HIP(hipMemcpy(s->inv2s.get(), ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
    if (s->q_pad > s->q) {
      AQ_HIP(hipMemcpy(s->sig2b.get() + s->q, ones.data(), (size_t)(s->q_pad - s->q) * sizeof(double), hipMemcpyHostToDevice));
      AQ_HIP(hipMemcpy(s->tau.get() + s->q, ones.data(), (size_t)(s->q_pad - s->q) * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  {
    AqScalars h;
    std::memset(&h, 0, sizeof(h));
    h.sig02_inv = pr->sig02_inv_vb;
    h.lentz_mask[0] = h.lentz_mask[1] = ~0ull;
    AQ_HIP(hipMemcpy(s->sc.get(), &h, sizeof(h), hipMemcpyHostToDevice));
  }
  aq_fill_args(s.get());

  // ---- host loop state, R/atlasqtl_global_local_core.R:71-123 ----
  if (!s->has_anneal) {
    s->annealing = false; s->c = s->c_s = 1.0; s->it_init = 1;
  } else {
    s->annealing = true;
    s->ladder = aq_ladder(s->anneal);
    s->c = s->ladder[0]; s->c_s = s->c;            // anneal_scale <- TRUE
    s->it_init = (int)std::llround(s->anneal[2]);
  }
  if (s->thinned) { s->times_conv_sched = {1, 5, 10, 50}; s->batch_conv_sched = {1, 10, 25, 50}; }
  else { s->times_conv_sched = {1}; s->batch_conv_sched = {1}; }
  s->ind_batch_conv = (int)s->batch_conv_sched.size() + 1;
  s->batch_conv = 1;
  s->sig2_zeta = 1.0 / (s->c * ((double)s->p + s->t02_inv));                       // update_sig2_c0_vb_(p, t02, c), :105
  s->vec_sum_log_det_zeta = -(double)s->q_total * (std::log(s->t02) + std::log((double)s->p + s->t02_inv));   // :107
  s->phase = 0;
  *out = s.release();
  return AQ_OK;
}

extern "C" void aq_vb_destroy(aq_vb_handle h) {
  if (!h) return;
  hipSetDevice(h->device);
  delete h;
}
