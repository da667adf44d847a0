// aq_vb.h -- the handle behind aq_vb_handle: the problem, the device-resident VB state and the run state of the sweep
// sequencing that replaces the reference's R-level loop (R/atlasqtl_global_local_core.R:125-386).  Shared by aq_vb_create.hip
// (which builds it), aq_vb_sweep.hip (which advances it) and aq_vb_query.hip (which reads it).
#pragma once
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "aq_internal.h"
#include "aq_plan.h"
#include "aq_core_sweep.h"
#include "aq_core_sweep_mis.h"
#include "aq_trait_wave.h"
#include "aq_vec_args.h"

// ------------------------------------------------------------------ state ----
// The launch plan (aq_plan.h: kernel, geometry, padded sizes; fixed when the handle is created) is the base; everything declared
// here is the problem, the device buffers and the run state.  The handle owns its device buffers: destroying it frees them.
struct aq_vb : AqPlan {
  int n, p, q, q_total, dmode, device, world, trait_offset = 0;
  // hyper / control
  double A2_inv, m0, nu, rho, t02, t02_inv, shr;
  bool has_anneal;
  int scheme = 0, df = 1;   // scheme 1 = global-only core (atlasqtl_global_core_); df of the horseshoe's half-t prior (1 or 3)
  double anneal[3];
  std::vector<double> ladder;
  double tol;
  int maxit;
  bool thinned, debug;
  // device buffers
  AqDev<double2> XA, XU;
  AqDev<double> G, Gx, R, gam, mu;
  AqDev<double> theta, sig2_theta, L, lam2_inv, Q, ppart;
  AqDev<double> eta_h, kappa_h, n0, nobs;
  AqDev<double> zeta, tau, sig2b, log_tau, eta_vb, kappa_vb;
  AqDev<double> coef, inv2s, cst, sums, rowA, rowGB;
  AqDev<double> Aarr, Barr, colApart;
  AqDev<double> GK;  // [ntile][nb][AQ_GK_STRIDE]
  AqDev<double> XR;  // [nb][NR][16] row-major SNP panels (gather source of the per-trait Gram corrections)
  AqDev<int> midx, mcnt4;   // per-trait lists of missing samples
  AqDev<int> mobs;   // wide split: 1 = the trait's list holds its observed samples (the shorter list), aq_k_gk_blocks_g
  AqDev<double> Pbuf, rnpart;
  AqDev<int> pflag;
  AqDev<double> Xcm, mis, XN;
  AqDev<int> done, errflag;
  bool pre_done = false;
  bool fused = false;    // look-ahead kernel: the pre-pass (A, b, sums of a) is computed inside the sweep kernel
  AqDev<double> red_own, ered_own, Hpart;   // the all-reduce payloads, unless the caller gave its own buffers
  double *red = nullptr, *ered = nullptr;   // the payloads in use: red_own / ered_own, or ext_reduce_main / ext_reduce_elbo
  AqDev<AqScalars> sc;
  int pblk = 0, nHchunk = 0, rows_per_chunk = 0;
  // argument blocks of the kernels, filled once by aq_fill_args when the handle is created; a launcher sets what varies per
  // launch (mode, c, sqrt_c, c_is_one, do_H, nseg, dbg)
  AqCoreArgs core_args = {};
  AqMisArgs mis_args = {};
  AqTwArgs tw_args = {};
  AqPrepass pre_args = {};
  AqQvec qv = {};
  AqPvec pv = {};
  // host-side loop state (R/atlasqtl_global_local_core.R:73-97,121-123)
  bool annealing = false;
  double c = 1.0, c_s = 1.0, sig2_zeta = 0.0, vec_sum_log_det_zeta = 0.0;
  int it_init = 1;
  std::vector<double> times_conv_sched;
  std::vector<int> batch_conv_sched;
  int ind_batch_conv = 0, batch_conv = 1;
  bool converged = false;
  double lb_new = -std::numeric_limits<double>::infinity(), lb_old = -std::numeric_limits<double>::infinity();
  int it = 0;
  int phase = 0;   // 0 start, 1 after init reduce, 2 sweep part A next, 3 after main reduce, 4 after elbo reduce
  bool has_missing = false;
  std::vector<int> trace_it;
  std::vector<double> trace_lb;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  double core_ms_acc = 0.0;
  int core_launches = 0;
  aq_shard_sorted *bf = nullptr;   // this rank's sorted PPIs between aq_vb_bfdr_begin and aq_vb_bfdr_end
  bool failed = false;
  int fail_code = AQ_ERR_NUMERIC;   // why the handle failed (reported again by every later advance)
  std::string fail_msg;
  bool errflag_forced = false;   // test hook aq_vb_debug_raise_errflag
  int budget = -1;
  std::string overrides;   // "NAME=value ..." of the AQ_* hooks the plan consulted and found set when the handle was created

  ~aq_vb() {   // events and the sorted shard; the AqDev members free themselves
    for (auto &e : ev) {
      hipEventDestroy(e.first);
      hipEventDestroy(e.second);
    }
    if (bf) aq_shard_free(bf);
  }
};

// elements of the exchange buffer Pbuf of a sample split: [ntile][2][parts][256]; wide: + the slot of the totals
inline size_t aq_pbuf_elems(const aq_vb &s) {
  const int parts = s.use_mis ? s.misC : s.laC + (s.la_wide ? 1 : 0);
  return (size_t)s.ntile * 2 * parts * 256;
}
// LDS bytes of the per-trait index lists [16][Mmax] (aq_k_gk_blocks, aq_core_sweep_mis_kernel)
inline size_t aq_midx_lds_bytes(int Mmax) { return (size_t)16 * Mmax * sizeof(unsigned short); }
// dynamic LDS bytes of the masked two-barrier kernel
inline size_t aq_mis_lds_bytes(int Mmax) {
  return (size_t)(8 * 256 + 11 * 256 + 5 * 256 + 8 * 4 * 16 + 2 * 256 * 17) * sizeof(double) + 16 * sizeof(int) + aq_midx_lds_bytes(Mmax);
}
