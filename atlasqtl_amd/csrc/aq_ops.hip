// aq_ops.hip -- the entries of libatlasqtl_hip.so that need no handle: error text, version, device count, the f64 MFMA
// layout probe, the planner without a device, the operator-level entries (coreDualLoop / coreDualMisLoop), the
// special-function evaluators and the debug hooks.  gfx950 only.  No CPU fallback: every compute entry fails loudly without
// a HIP device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aq_vb.h"
#include "aq_gram_loop.h"
#include "aq_special.h"

// ------------------------------------------------------------------ errors ----
static thread_local std::string g_err;
int aq_fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
std::atomic<int64_t> aq_live_device_bytes{0};

extern "C" const char *aq_last_error(void) { return g_err.c_str(); }
extern "C" const char *aq_version(void) { return "atlasqtl_hip 0.1.0 (gfx950)"; }
extern "C" int aq_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int aq_need_device(int device) {
  int n = aq_device_count();
  if (n <= 0)
    return aq_fail(AQ_ERR_DEVICE, "no HIP device visible: libatlasqtl_hip has no CPU fallback (MI355X / gfx950 required)");
  if (device < 0 || device >= n) return aq_fail(AQ_ERR_ARG, "device ordinal out of range");
  AQ_HIP(hipSetDevice(device));
  return AQ_OK;
}

// ------------------------------------------------- f64 MFMA D-layout probe ----
// D = A(16x4) * B(4x16) with A[i][k] = (k==0 ? i : 0), B[0][j] = 1  =>  D[i][j] = i.
// Reading reg 1 of lane 16 tells which row the (reg, lane>>4) pair maps to.
__global__ void aq_k_probe_dlayout(double *out) {
  int lane = threadIdx.x & 63;
  double av = ((lane >> 4) == 0) ? (double)(lane & 15) : 0.0;
  double bv = ((lane >> 4) == 0) ? 1.0 : 0.0;
  aq_d4 acc = {0, 0, 0, 0};
  acc = aq_mfma(av, bv, acc);
  for (int r = 0; r < 4; r++) out[lane * 4 + r] = acc[r];
}
static int g_dmode = -1;
int aq_probe_dmode(int *dmode) {
  if (g_dmode >= 0) {
    *dmode = g_dmode;
    return AQ_OK;
  }
  AqDev<double> d;
  AQ_TRY(d.alloc(256));
  hipLaunchKernelGGL(aq_k_probe_dlayout, dim3(1), dim3(64), 0, 0, d.get());
  double h[256];
  AQ_HIP(hipMemcpy(h, d.get(), sizeof(h), hipMemcpyDeviceToHost));
  d.reset();
  // lane 16 (g = 1), reg 1: row = g + 4*reg = 5 (mode 0)  or  4*g + reg = 5 (mode 1)?  ambiguous -> use lane 16 reg 0
  // lane 16, reg 0: mode 0 -> row 1, mode 1 -> row 4.
  double v = h[16 * 4 + 0];
  int mode;
  if (v == 1.0) mode = 0;
  else if (v == 4.0) mode = 1;
  else return aq_fail(AQ_ERR_DEVICE, "unexpected v_mfma_f64_16x16x4 accumulator layout (probe value " + std::to_string(v) + ")");
  // full check of the chosen map
  for (int lane = 0; lane < 64; lane++)
    for (int r = 0; r < 4; r++) {
      int g = lane >> 4;
      int row = mode ? 4 * g + r : 4 * r + g;
      if (h[lane * 4 + r] != (double)row)
        return aq_fail(AQ_ERR_DEVICE, "v_mfma_f64_16x16x4 accumulator layout does not match either known map");
    }
  g_dmode = mode;
  *dmode = mode;
  return AQ_OK;
}

// the f64 MFMA accumulator map that the band, GRM and operator kernels of the prepare side are written for
// (row = (lane >> 4) + 4 reg), checked on the device
int aq_need_acc_layout(const char *who) {
  int dmode = 0;
  AQ_TRY(aq_probe_dmode(&dmode));
  if (dmode != 0)
    return aq_fail(AQ_ERR_DEVICE, std::string(who) + ": the band kernel is written for the accumulator map row = (lane >> 4) + 4 reg "
                                                     "of v_mfma_f64_16x16x4_f64, which this device does not have");
  return AQ_OK;
}

// The planner without a device: the plan fields of aq_vb_status for given sizes, missingness counts, CU count and memory, with
// the hooks taken from `overrides` ("NAME=value NAME=value") and never from the process environment.
extern "C" int aq_plan_query(int32_t n, int32_t p, int32_t q, int32_t max_missing, int32_t max_short_list, int32_t ncu, int64_t total_bytes,
                             const char *overrides, aq_vb_status *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_plan_query: NULL argument");
  std::memset(out, 0, sizeof(*out));
  if (n < 2 || p < 1 || q < 1) return aq_fail(AQ_ERR_ARG, "aq_plan_query: n >= 2, p >= 1, q >= 1 required");
  if (ncu < 1 || max_short_list < 0 || max_short_list > max_missing || max_missing > n)
    return aq_fail(AQ_ERR_ARG, "aq_plan_query: ncu >= 1 and 0 <= max_short_list <= max_missing <= n required");
  std::vector<std::pair<std::string, std::string>> hooks;
  const std::string ov = overrides ? overrides : "";
  for (size_t a = 0; a < ov.size();) {
    size_t b = ov.find(' ', a);
    if (b == std::string::npos) b = ov.size();
    const size_t eq = ov.find('=', a);
    if (b > a) {
      if (eq == std::string::npos || eq >= b || eq == a) return aq_fail(AQ_ERR_ARG, "aq_plan_query: overrides must read \"NAME=value NAME=value\"");
      hooks.push_back({ov.substr(a, eq - a), ov.substr(eq + 1, b - eq - 1)});
    }
    a = b + 1;
  }
  const AqEnv env = [&hooks](const char *name) -> const char * {
    for (auto &hk : hooks)
      if (hk.first == name) return hk.second.c_str();
    return nullptr;
  };
  AqPlanInput in;
  in.n = n; in.p = p; in.q = q;
  in.has_missing = max_missing > 0; in.max_missing = max_missing; in.max_short_list = max_short_list;
  in.ncu = ncu; in.total_bytes = total_bytes;
  AqPlan plan;
  std::string err;
  const int rc = aq_make_plan(in, env, &plan, &err);
  if (rc == AQ_ERR_DEVICE)   // the planner's only device error: the memory size is unknown where the wide split needs it
    return aq_fail(AQ_ERR_ARG, "aq_plan_query: the wide sample split (n > 10240 or AQ_LA_C >= 9) needs total_bytes, the device's memory size");
  if (rc != AQ_OK) return aq_fail(rc, err);
  aq_plan_to_status(plan, out);
  return AQ_OK;
}

// ------------------------------------------------- operator-level entries ----
static int aq_gram_common(bool mis, const double *cp_X, const double *const *cp_X_rm, const double *cp_Y_X, double *gam_vb,
                          const double *lP, const double *l1, double log_sig2_inv_vb, const double *log_tau_vb,
                          double *m1_beta, double *cp_betaX_X, double *mu_beta_vb, const double *sig2_beta_vb,
                          const double *tau_vb, const int32_t *shuffled_ind, int32_t n_ind, const int32_t *sample_q,
                          int32_t n_q, double c, int32_t p, int32_t q) {
  if (!cp_X || !cp_Y_X || !gam_vb || !lP || !l1 || !log_tau_vb || !m1_beta || !cp_betaX_X || !mu_beta_vb || !sig2_beta_vb ||
      !tau_vb || (mis && !cp_X_rm))
    return aq_fail(AQ_ERR_ARG, "aq_core_dual_loop: NULL argument");
  if (p < 1 || q < 1 || n_ind < 0 || n_q < 0) return aq_fail(AQ_ERR_ARG, "aq_core_dual_loop: bad sizes");
  if ((n_ind > 0 && !shuffled_ind) || (n_q > 0 && !sample_q)) return aq_fail(AQ_ERR_ARG, "aq_core_dual_loop: NULL index vector");
  for (int i = 0; i < n_ind; i++)
    if (shuffled_ind[i] < 0 || shuffled_ind[i] >= p) return aq_fail(AQ_ERR_ARG, "shuffled_ind out of range [0, p)");
  {
    std::vector<char> seen((size_t)q, 0);
    for (int i = 0; i < n_q; i++) {
      if (sample_q[i] < 0 || sample_q[i] >= q) return aq_fail(AQ_ERR_ARG, "sample_q out of range [0, q)");
      if (seen[sample_q[i]]) return aq_fail(AQ_ERR_ARG, "sample_q holds a repeated trait index");
      seen[sample_q[i]] = 1;
    }
  }
  AQ_TRY(aq_need_device(0));
  if (n_ind == 0 || n_q == 0) return AQ_OK;   // empty index vectors: nothing to do (the reference's loops do not execute)


  size_t pp = (size_t)p * p, pq = (size_t)p * q;
  // a device copy of `count` elements of src
  auto up = [](const auto *src, size_t count, auto *dst) -> int {
    AQ_TRY(dst->alloc(count));
    AQ_HIP(hipMemcpy(dst->get(), src, count * sizeof(*src), hipMemcpyHostToDevice));
    return AQ_OK;
  };
  AqGramArgs a;
  std::memset(&a, 0, sizeof(a));
  AqDev<double> d_cpX, d_cpYX, d_gam, d_lP, d_l1, d_lt, d_m1, d_bx, d_mu, d_s2, d_tau;
  AqDev<int32_t> d_si, d_sq;
  AQ_TRY(up(cp_X, pp, &d_cpX));
  AQ_TRY(up(cp_Y_X, pq, &d_cpYX));
  AQ_TRY(up(gam_vb, pq, &d_gam));
  AQ_TRY(up(lP, pq, &d_lP));
  AQ_TRY(up(l1, pq, &d_l1));
  AQ_TRY(up(log_tau_vb, (size_t)q, &d_lt));
  AQ_TRY(up(m1_beta, pq, &d_m1));
  AQ_TRY(up(cp_betaX_X, pq, &d_bx));
  AQ_TRY(up(mu_beta_vb, pq, &d_mu));
  AQ_TRY(up(sig2_beta_vb, mis ? pq : (size_t)q, &d_s2));
  AQ_TRY(up(tau_vb, (size_t)q, &d_tau));
  AQ_TRY(up(shuffled_ind, (size_t)n_ind, &d_si));
  AQ_TRY(up(sample_q, (size_t)n_q, &d_sq));
  std::vector<AqDev<double>> d_rm;
  AqDev<const double *> d_rm_arr;
  if (mis) {
    std::vector<const double *> hp((size_t)q, nullptr);
    d_rm.resize((size_t)q);
    for (int k = 0; k < q; k++) {
      if (!cp_X_rm[k]) return aq_fail(AQ_ERR_ARG, "cp_X_rm holds a NULL matrix");
      AQ_TRY(up(cp_X_rm[k], pp, &d_rm[k]));
      hp[k] = d_rm[k].get();
    }
    AQ_TRY(up(hp.data(), (size_t)q, &d_rm_arr));
  }
  a.cp_X = d_cpX.get(); a.cp_X_rm = d_rm_arr.get(); a.cp_Y_X = d_cpYX.get(); a.gam_vb = d_gam.get(); a.log_Phi = d_lP.get();
  a.log_1mPhi = d_l1.get(); a.log_sig2_inv_vb = log_sig2_inv_vb; a.log_tau_vb = d_lt.get(); a.m1_beta = d_m1.get();
  a.cp_betaX_X = d_bx.get(); a.mu_beta_vb = d_mu.get(); a.sig2_beta_vb = d_s2.get(); a.tau_vb = d_tau.get();
  a.shuffled_ind = d_si.get(); a.n_ind = n_ind; a.sample_q = d_sq.get(); a.n_q = n_q;
  a.c = c; a.p = p; a.q = q;
  int grid = n_q < 2048 ? n_q : 2048;
  if (mis) hipLaunchKernelGGL((aq_gram_loop_kernel<true>), dim3(grid), dim3(256), 0, 0, a);
  else hipLaunchKernelGGL((aq_gram_loop_kernel<false>), dim3(grid), dim3(256), 0, 0, a);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(gam_vb, d_gam.get(), pq * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(m1_beta, d_m1.get(), pq * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(cp_betaX_X, d_bx.get(), pq * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(mu_beta_vb, d_mu.get(), pq * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return aq_fail(AQ_ERR_DEVICE, std::string("aq_core_dual_loop: ") + hipGetErrorString(e));
  return AQ_OK;
}

extern "C" int aq_core_dual_loop(const double *cp_X, const double *cp_Y_X, double *gam_vb, const double *lP, const double *l1,
                                 double log_sig2_inv_vb, const double *log_tau_vb, double *m1_beta, double *cp_betaX_X,
                                 double *mu_beta_vb, const double *sig2_beta_vb, const double *tau_vb,
                                 const int32_t *shuffled_ind, int32_t n_ind, const int32_t *sample_q, int32_t n_q, double c,
                                 int32_t p, int32_t q) {
  return aq_gram_common(false, cp_X, nullptr, cp_Y_X, gam_vb, lP, l1, log_sig2_inv_vb, log_tau_vb, m1_beta, cp_betaX_X,
                        mu_beta_vb, sig2_beta_vb, tau_vb, shuffled_ind, n_ind, sample_q, n_q, c, p, q);
}
extern "C" int aq_core_dual_mis_loop(const double *cp_X, const double *const *cp_X_rm, const double *cp_Y_X, double *gam_vb,
                                     const double *lP, const double *l1, double log_sig2_inv_vb, const double *log_tau_vb,
                                     double *m1_beta, double *cp_betaX_X, double *mu_beta_vb, const double *sig2_beta_vb,
                                     const double *tau_vb, const int32_t *shuffled_ind, int32_t n_ind,
                                     const int32_t *sample_q, int32_t n_q, double c, int32_t p, int32_t q) {
  return aq_gram_common(true, cp_X, cp_X_rm, cp_Y_X, gam_vb, lP, l1, log_sig2_inv_vb, log_tau_vb, m1_beta, cp_betaX_X,
                        mu_beta_vb, sig2_beta_vb, tau_vb, shuffled_ind, n_ind, sample_q, n_q, c, p, q);
}

// ------------------------------------------------------------- test hooks ----
extern "C" int aq_vb_debug_raise_errflag(aq_vb_handle s) {
  if (!s || !s->errflag.get()) return aq_fail(AQ_ERR_ARG, "NULL handle");
  AQ_HIP(hipSetDevice(s->device));
  int one = 1;
  AQ_HIP(hipMemcpy(s->errflag.get(), &one, sizeof(int), hipMemcpyHostToDevice));
  s->errflag_forced = true;
  return AQ_OK;
}
extern "C" int64_t aq_debug_live_device_bytes(void) { return aq_live_device_bytes.load(); }

// What aq_vb_create built once for this handle, read back as it lies in device memory: copies only, no kernel, no lifetime
// changed (a buffer the handle has already released reads as length 0).
extern "C" int64_t aq_vb_debug_get_setup(aq_vb_handle s, int32_t which, void *buf, int64_t cap_bytes) {
  if (!s) return -(int64_t)aq_fail(AQ_ERR_ARG, "aq_vb_debug_get_setup: NULL handle");
  if (which < 0 || which >= AQ_SETUP_COUNT) return -(int64_t)aq_fail(AQ_ERR_ARG, "aq_vb_debug_get_setup: which out of range");
  if (cap_bytes < 0 || (cap_bytes > 0 && !buf)) return -(int64_t)aq_fail(AQ_ERR_ARG, "aq_vb_debug_get_setup: NULL buffer or negative capacity");
  const int32_t geo[AQ_SETUP_GEOMETRY_LEN] = {s->nb, s->ntile, s->n_pad, s->p_pad, s->q_pad, s->NR, s->Mmax, s->dmode, s->use_la ? 1 : 0,
                                              s->la_mask ? 1 : 0, s->la_wide ? 1 : 0, s->use_mis ? 1 : 0, s->use_tw ? 1 : 0};
  if (which == AQ_SETUP_GEOMETRY) {
    if (cap_bytes >= (int64_t)sizeof(geo)) std::memcpy(buf, geo, sizeof(geo));
    return (int64_t)sizeof(geo);
  }
  const size_t xpanel = (size_t)s->nb * (s->n_pad / 16) * 128 * sizeof(double2), tile16 = (size_t)s->ntile * 16;
  const void *src = nullptr;
  size_t bytes = 0;
  switch (which) {
    case AQ_SETUP_XA: src = s->use_tw ? nullptr : s->XA.get(); bytes = xpanel; break;
    case AQ_SETUP_XU: src = s->use_tw ? nullptr : s->XU.get(); bytes = xpanel; break;
    case AQ_SETUP_XR: src = s->XR.get(); bytes = (size_t)s->nb * s->NR * 16 * sizeof(double); break;
    case AQ_SETUP_G: src = s->use_tw ? nullptr : s->G.get(); bytes = (size_t)s->nb * 256 * sizeof(double); break;
    case AQ_SETUP_GX: src = s->use_tw ? nullptr : s->Gx.get(); bytes = (size_t)s->nb * 256 * sizeof(double); break;
    case AQ_SETUP_GK: src = s->GK.get(); bytes = (size_t)s->ntile * s->nb * AQ_GK_STRIDE * sizeof(double); break;
    case AQ_SETUP_MIDX: src = s->midx.get(); bytes = tile16 * s->Mmax * sizeof(int); break;
    case AQ_SETUP_MCNT4: src = s->mcnt4.get(); bytes = tile16 * sizeof(int); break;
    case AQ_SETUP_MOBS: src = s->mobs.get(); bytes = tile16 * sizeof(int); break;
    case AQ_SETUP_MIS: src = s->mis.get(); bytes = tile16 * s->n_pad * sizeof(double); break;
    case AQ_SETUP_R: src = s->R.get(); bytes = tile16 * s->n_pad * sizeof(double); break;
    case AQ_SETUP_GAM: src = s->gam.get(); bytes = tile16 * s->p_pad * sizeof(double); break;
    case AQ_SETUP_MU: src = s->mu.get(); bytes = tile16 * s->p_pad * sizeof(double); break;
  }
  if (!src) return 0;
  if (cap_bytes >= (int64_t)bytes) {
    hipError_t e = hipSetDevice(s->device);
    if (e == hipSuccess) e = hipMemcpy(buf, src, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return -(int64_t)aq_fail(AQ_ERR_DEVICE, std::string("aq_vb_debug_get_setup: ") + hipGetErrorString(e));
  }
  return (int64_t)bytes;
}

// one element of the test hook, compiled for host and device from the same header the kernels use
__host__ __device__ static inline bool aq_special_one(int which, double x, double x2, double *out) {
  double a_, b_, c_, d_;
  switch (which) {
    case 0: *out = aq_log_ndtr(x); return true;
    case 1: *out = aq_digamma(x); return true;
    case 2: *out = aq_expint_e1_small(x); return true;
    case 3: *out = aq_gamma_inc_upper(x2, x); return true;
    case 4: *out = aq_sigmoid_neg(x); return true;
    case 5: aq_log_ndtr_pair(x, &a_, &b_); *out = a_; return true;
    case 6: aq_log_ndtr_pair(x, &a_, &b_); *out = b_; return true;
    case 7: aq_probit_terms(x, &a_, &b_, &c_, &d_); *out = c_; return true;
    case 8: aq_probit_terms(x, &a_, &b_, &c_, &d_); *out = d_; return true;
    case 9: *out = aq_erfcx_pos(x); return true;
    case 10: aq_probit_A_imr(x, &a_, &b_, &c_, &d_); *out = a_; return true;
    case 11: aq_probit_A_imr(x, &a_, &b_, &c_, &d_); *out = b_; return true;
    case 12: aq_probit_A_imr(x, &a_, &b_, &c_, &d_); *out = c_; return true;
    case 13: *out = aq_sigmoid_neg_fast(x); return true;
    // compute_integral_hs_(alpha = df, beta = L df, m, n, Q(L)) for the horseshoe's df = 5 (14: m = n = 3, 15: m = 3, n = 2) and
    // df = 7 (16: m = n = 4, 17: m = 4, n = 3); x = L, x2 = Q_approx(L)
    case 14: *out = aq_hs_integral(5.0, 5.0 * x, 3, 3, x2); return true;
    case 15: *out = aq_hs_integral(5.0, 5.0 * x, 3, 2, x2); return true;
    case 16: *out = aq_hs_integral(7.0, 7.0 * x, 4, 4, x2); return true;
    case 17: *out = aq_hs_integral(7.0, 7.0 * x, 4, 3, x2); return true;
    // the table-driven probit terms of the sweep kernel's helper wave (aq_probit_tab.h): A, imr1, imr0
    // update_annealed_lam2_inv_vb_ for df = 3, 5, 7 (R/update_vb.R:76-81): x = L_vb, x2 = c
    case 21: *out = aq_annealed_lam2_inv_df(x, x2, 3.0); return true;
    case 22: *out = aq_annealed_lam2_inv_df(x, x2, 5.0); return true;
    case 23: *out = aq_annealed_lam2_inv_df(x, x2, 7.0); return true;
    case 18: aq_probit_A_imr_tab(x, aq_pt_table(), &a_, &b_, &c_); *out = a_; return true;
    case 19: aq_probit_A_imr_tab(x, aq_pt_table(), &a_, &b_, &c_); *out = b_; return true;
    case 20: aq_probit_A_imr_tab(x, aq_pt_table(), &a_, &b_, &c_); *out = c_; return true;
    // log Phi(x), log(1 - Phi(x)) from the tables, as the ELBO pass takes them (aq_log_ndtr_pair_tab)
    case 24: aq_log_ndtr_pair_tab(x, aq_pt_table(), aq_ptn_table(), &a_, &b_); *out = a_; return true;
    case 25: aq_log_ndtr_pair_tab(x, aq_pt_table(), aq_ptn_table(), &a_, &b_); *out = b_; return true;
    // Phi^-1(x) for 0 < x <= 1/2, as the rank-based inverse normal transform of Y takes it (aq_ytrans_kernels.h)
    case 26: *out = aq_ndtri(x); return true;
    default: return false;
  }
}

extern "C" int aq_special_eval(int32_t which, const double *x, const double *x2, double *out, int64_t len) {
  if (!x || !out || len < 0) return aq_fail(AQ_ERR_ARG, "aq_special_eval: bad argument");
  if ((which == 3 || (which >= 14 && which <= 17) || (which >= 21 && which <= 23)) && !x2) return aq_fail(AQ_ERR_ARG, "aq_special_eval: x2 required");
  for (int64_t i = 0; i < len; i++)
    if (!aq_special_one(which, x[i], x2 ? x2[i] : 0.0, &out[i])) return aq_fail(AQ_ERR_ARG, "aq_special_eval: unknown function id");
  return AQ_OK;
}

__global__ void aq_k_special_eval(int which, const double *x, const double *x2, double *out, long long len) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < len) aq_special_one(which, x[i], x2 ? x2[i] : 0.0, &out[i]);
}

extern "C" int aq_special_eval_device(int32_t which, const double *x, const double *x2, double *out, int64_t len, int32_t device) {
  if (!x || !out || len < 0) return aq_fail(AQ_ERR_ARG, "aq_special_eval_device: bad argument");
  if (which < 0 || which > 26) return aq_fail(AQ_ERR_ARG, "aq_special_eval_device: unknown function id");
  if ((which == 3 || (which >= 14 && which <= 17) || (which >= 21 && which <= 23)) && !x2) return aq_fail(AQ_ERR_ARG, "aq_special_eval_device: x2 required");
  AQ_TRY(aq_need_device(device));
  if (len == 0) return AQ_OK;
  AqDev<double> dx, dx2, dout;
  AQ_TRY(dx.alloc((size_t)len));
  AQ_TRY(dout.alloc((size_t)len));
  AQ_HIP(hipMemcpy(dx.get(), x, len * sizeof(double), hipMemcpyHostToDevice));
  if (x2) {
    AQ_TRY(dx2.alloc((size_t)len));
    AQ_HIP(hipMemcpy(dx2.get(), x2, len * sizeof(double), hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(aq_k_special_eval, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, 0, which, dx.get(), dx2.get(), dout.get(), (long long)len);
  AQ_HIP(hipMemcpy(out, dout.get(), len * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}

extern "C" int aq_q_approx_vec(const double *x, double *out, int64_t len, int32_t *iters) {
  if (!x || !out || len < 0) return aq_fail(AQ_ERR_ARG, "aq_q_approx_vec: bad argument");
  unsigned long long m0 = ~0ull, m1 = ~0ull;
  bool any = false;
  for (int64_t i = 0; i < len; i++) {
    if (x[i] > 1.0) {
      AqLentz s;
      aq_lentz_init(&s);
      unsigned long long a0 = 0, a1 = 0;
      for (int it = 0; it < 128; it++) {
        double d = aq_lentz_step(&s, x[i], it + 2);
        if (d < 1e-7) { if (it < 64) a0 |= 1ull << it; else a1 |= 1ull << (it - 64); }
      }
      m0 &= a0; m1 &= a1;
      any = true;
    }
  }
  int nit = 0;
  if (any) nit = m0 ? __builtin_ffsll((long long)m0) : (m1 ? 64 + __builtin_ffsll((long long)m1) : 129);
  for (int64_t i = 0; i < len; i++) {
    if (x[i] <= 1.0) {
      out[i] = aq_expint_e1_small(x[i]) * exp(x[i]);
    } else {
      AqLentz s;
      aq_lentz_init(&s);
      for (int it = 0; it < nit; it++) aq_lentz_step(&s, x[i], it + 2);
      out[i] = aq_lentz_finish(&s, x[i]);
    }
  }
  if (iters) *iters = nit;
  return AQ_OK;
}
