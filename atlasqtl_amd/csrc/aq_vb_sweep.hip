// aq_vb_sweep.hip -- the sweep sequencing that replaces the reference's R-level loop (R/atlasqtl_global_local_core.R:125-386):
// the three core-kernel launchers, the pre-pass, parts A and B of a sweep, the ELBO, the state machine behind aq_vb_advance
// and the run entries.  The argument blocks of the kernels live in the handle (aq_vb_create.hip::aq_fill_args); a launcher
// sets only what varies per launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "aq_vb.h"
#include "aq_launch_la.h"
#include "aq_sweep_kernels.h"

bool aq_all_equal_1(double c) { return std::fabs(c - 1.0) < 1.5e-8; }   // isTRUE(all.equal(c, 1)), R/update_vb.R:219

// ---- the three core-kernel dispatches ---------------------------------------------------------------------------------------
// Each walks the instance set of aq_plan_const.h at compile time (aq_first_arm), instantiates what is built and launches the
// instance a request names -- or, run dry, writes that instance's own template parameters and touches no device:
// aq_instance_query.  The look-ahead kernel's walk is aq_la_unit (aq_launch_la_unit.h), in its five units.
struct AqFbRun { const void *args; unsigned ntile; size_t lds; aq_kernel_instance *dry; };   // the two fallback kernels

static int aq_tw_dispatch(int NE, int WPT, const AqFbRun &r) {
  constexpr int NNE = sizeof AQ_TW_NE / sizeof *AQ_TW_NE, NWPT = sizeof AQ_TW_WPT / sizeof *AQ_TW_WPT;
  const int rc = aq_first_arm<NNE * NWPT>([&](auto cell) -> int {
    constexpr int NE_ = AQ_TW_NE[decltype(cell)::value / NWPT], WPT_ = AQ_TW_WPT[decltype(cell)::value % NWPT];
    if constexpr (aq_tw_built(NE_, WPT_)) {
      if (NE != NE_ || WPT != WPT_) return -1;
      if (r.dry) { r.dry->ne = NE_; r.dry->wpt = WPT_; return AQ_OK; }
      AQ_HIP(hipFuncSetAttribute((const void *)aq_trait_wave_kernel<NE_, WPT_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.lds));
      hipLaunchKernelGGL((aq_trait_wave_kernel<NE_, WPT_>), dim3(r.ntile * WPT_), dim3(1024), r.lds, 0, *(const AqTwArgs *)r.args);
      return AQ_OK;
    }
    return -1;
  });
  return rc >= 0 ? rc : aq_fail(AQ_ERR_UNSUPPORTED, "no generic kernel instantiation for this n");
}

static int aq_mis_dispatch(int NT, unsigned parts, const AqFbRun &r) {
  const int rc = aq_first_arm<sizeof AQ_MIS_NT / sizeof *AQ_MIS_NT>([&](auto cell) -> int {
    constexpr int NT_ = AQ_MIS_NT[decltype(cell)::value];
    if (NT != NT_) return -1;
    if (r.dry) { r.dry->nt = NT_; return AQ_OK; }
    AQ_HIP(hipFuncSetAttribute((const void *)aq_core_sweep_mis_kernel<NT_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.lds));
    hipLaunchKernelGGL((aq_core_sweep_mis_kernel<NT_>), dim3(r.ntile * parts), dim3(512), r.lds, 0, *(const AqMisArgs *)r.args);
    return AQ_OK;
  });
  return rc >= 0 ? rc : aq_fail(AQ_ERR_UNSUPPORTED, "no masked MFMA kernel instantiation for this n");
}

// the look-ahead request that the instance fields of a status name (aq_plan_to_status wrote them, or a caller of aq_instance_query)
static AqLaRequest aq_la_request(const aq_vb_status &q) {
  return {q.tiles_matrix, q.tiles_matrix2, q.tiles_recurrence, q.tiles_per_group, (q.instance_flags & 4) != 0, (q.instance_flags & 1) != 0,
          (q.instance_flags & 2) != 0};
}
static int aq_la_dispatch(const AqLaRequest &rq, unsigned grid, const AqCoreArgs *a, aq_kernel_instance *dry) {
  if (aq_la_launch(rq, grid, 0, a, dry) != 0) return aq_fail(AQ_ERR_UNSUPPORTED, "no look-ahead kernel instantiation for this n");
  return AQ_OK;
}

extern "C" int aq_instance_query(const aq_vb_status *request, int32_t ne, int32_t wpt, aq_kernel_instance *out) {
  if (!request || !out) return aq_fail(AQ_ERR_ARG, "aq_instance_query: NULL argument");
  std::memset(out, 0, sizeof(*out));
  aq_kernel_instance got = {};
  got.core_kernel = request->core_kernel;
  if (request->core_kernel == 3) AQ_TRY(aq_mis_dispatch(request->tiles_matrix, 0, AqFbRun{nullptr, 0, 0, &got}));
  else if (request->core_kernel == 2) AQ_TRY(aq_tw_dispatch(ne, wpt, AqFbRun{nullptr, 0, 0, &got}));
  else if (request->core_kernel == 0) AQ_TRY(aq_la_dispatch(aq_la_request(*request), 0, nullptr, &got));
  else return aq_fail(AQ_ERR_ARG, "aq_instance_query: core_kernel is 0 (look-ahead), 2 (generic) or 3 (masked)");
  *out = got;
  return AQ_OK;
}

static int aq_launch_tw(aq_vb *s, int mode, double c) {
  AqTwArgs &t = s->tw_args;
  t.c = c; t.mode = mode;
  size_t lds = (size_t)(s->tw_ns * s->n_pad + 8 * 256 + 32) * sizeof(double);
  AQ_TRY(aq_tw_dispatch(s->NE, s->WPT, AqFbRun{&t, (unsigned)s->ntile, lds, nullptr}));
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

static int aq_launch_mis(aq_vb *s, int mode, double c) {
  AqMisArgs &t = s->mis_args;
  const int nseg = (mode == 0 && s->misC == 1 && s->chain > 1) ? s->chain : 1;
  t.c = c; t.mode = mode; t.nseg = nseg;
  if (nseg > 1) AQ_HIP(hipMemsetAsync(s->done.get(), 0, (size_t)s->ntile * sizeof(int), 0));
  if (s->misC > 1) AQ_HIP(hipMemsetAsync(s->pflag.get(), 0, (size_t)s->ntile * s->misC * sizeof(int), 0));
  AQ_TRY(aq_mis_dispatch(s->NT, (unsigned)(s->misC * nseg), AqFbRun{&t, (unsigned)s->ntile, aq_mis_lds_bytes(s->Mmax), nullptr}));
  if (nseg > 1)
    hipLaunchKernelGGL(aq_k_combine_segment_sums6, dim3((s->q_pad + 255) / 256), dim3(256), 0, 0, s->sums.get(), s->q_pad, nseg);
  if (s->misC > 1)
    hipLaunchKernelGGL(aq_k_sum_parts, dim3((s->q_pad + 255) / 256), dim3(256), 0, 0, s->rnpart.get(), s->sums.get() + (size_t)4 * s->q_pad, s->misC, s->q_pad);
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

// AQ_DIAG_DUMP=<file> with a -DAQ_DIAG_TIME build: per-role wait / total cycles of sweep 15.  The counters of a sweep go into
// one process-wide buffer: per-wave counters of up to 32 nwg workgroups + the timeline of workgroup 0.
static int aq_diag_begin(unsigned nwg, long long **dbg) {
  static AqDev<long long> *dbg_buf = new AqDev<long long>();   // never destroyed: it would outlive the HIP runtime at exit
  static size_t dbg_cap = 0;
  const size_t dbg_n = (size_t)32 * nwg * 8 * 3 + 8 * 32 * 8;
  if (dbg_n > dbg_cap) {
    dbg_cap = 0;
    AQ_TRY(dbg_buf->alloc(dbg_n));
    dbg_cap = dbg_n;
  }
  AQ_HIP(hipMemsetAsync(dbg_buf->get(), 0, dbg_n * sizeof(long long), 0));
  *dbg = dbg_buf->get();
  return AQ_OK;
}
static int aq_diag_dump(const char *dump, const long long *dbg, unsigned grid) {
  AQ_HIP(hipDeviceSynchronize());
  std::vector<long long> h((size_t)grid * 24 + 8 * 32 * 8);
  AQ_HIP(hipMemcpy(h.data(), dbg, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
  if (FILE *f = fopen(dump, "w")) {
    for (unsigned b = 0; b < grid; b++)
      for (int w = 0; w < 8; w++)
        fprintf(f, "%u %d %lld %lld %lld\n", b, w, h[((size_t)b * 8 + w) * 3], h[((size_t)b * 8 + w) * 3 + 1], h[((size_t)b * 8 + w) * 3 + 2]);
    fclose(f);
  }
  if (FILE *f = fopen((std::string(dump) + ".timeline").c_str(), "w")) {   // workgroup 0, phases 64 .. 95: wave, phase, 4 marks
    const long long *t = h.data() + (size_t)grid * 24;
    for (int w = 0; w < 8; w++)
      for (int i = 0; i < 32; i++)
        fprintf(f, "%d %d %lld %lld %lld %lld %lld %lld %lld\n", w, 64 + i, t[(w * 32 + i) * 8], t[(w * 32 + i) * 8 + 1], t[(w * 32 + i) * 8 + 2],
                t[(w * 32 + i) * 8 + 3], t[(w * 32 + i) * 8 + 4], t[(w * 32 + i) * 8 + 5], t[(w * 32 + i) * 8 + 6]);
    fclose(f);
  }
  return AQ_OK;
}

static int aq_launch_core(aq_vb *s, int mode, double c) {
  hipEvent_t e0, e1;
  AQ_HIP(hipEventCreate(&e0));
  AQ_HIP(hipEventCreate(&e1));
  AQ_HIP(hipEventRecord(e0, 0));
  if (s->use_mis) {
    AQ_TRY(aq_launch_mis(s, mode, c));
  } else if (s->use_tw) {
    AQ_TRY(aq_launch_tw(s, mode, c));
  } else if (s->use_la) {
    AqCoreArgs &a = s->core_args;
    a.mode = mode; a.c = c; a.sqrt_c = std::sqrt(c);
    a.c_is_one = aq_all_equal_1(c) ? 1 : 0;
    const unsigned nwg = (unsigned)(s->ntile / s->TT);
    if (s->laC > 1 && (!a.Pbuf || !a.rnpart || !a.errflag)) return aq_fail(AQ_ERR_DEVICE, "sample split without its exchange buffers");
    if (s->laC > 1 && mode == 0)   // the exchange slots start with tag 0 (aq_core_sweep_la.h, split_exchange)
      AQ_HIP(hipMemsetAsync(s->Pbuf.get(), 0, aq_pbuf_elems(*s) * sizeof(double), 0));
    a.dbg = nullptr;
    const char *dump = getenv("AQ_DIAG_DUMP");
    if (dump && mode == 0) AQ_TRY(aq_diag_begin(nwg, &a.dbg));
    const bool chained = (mode == 0 && s->chain > 1);
    a.nseg = chained ? s->chain : 1;
    if (chained) AQ_HIP(hipMemsetAsync(s->done.get(), 0, (size_t)s->ntile * sizeof(int), 0));
    // chained-segment launch: chain * nwg workgroups, workgroup s*nwg + k = SNP segment s of trait-tile group k
    const unsigned grid = chained ? (unsigned)((long long)s->chain * nwg) : nwg * (unsigned)s->laC;
    // One instance per handle for annealed and post-annealing sweeps alike: with the probit tables an annealed entry costs the
    // same three polynomials as any other (round 2 swapped to a (NT, NT, 3) geometry for the annealed sweeps).
    aq_vb_status st;
    aq_plan_to_status(*s, &st);            // the instance in the terms of aq_vb_status ...
    AqLaRequest rq = aq_la_request(st);
    rq.seg = chained;                      // ... but for SEG: the ELBO-only launch (mode 1) of a chained plan is not chained
    AQ_TRY(aq_la_dispatch(rq, grid, &a, nullptr));
    if (chained) {
      if (s->la_mask) hipLaunchKernelGGL(aq_k_combine_segment_sums6, dim3((s->q_pad + 255) / 256), dim3(256), 0, 0, s->sums.get(), s->q_pad, s->chain);
      else hipLaunchKernelGGL(aq_k_combine_segment_sums, dim3((s->q_pad + 255) / 256), dim3(256), 0, 0, s->sums.get(), s->q_pad, s->chain);
    }
    if (s->laC > 1)
      hipLaunchKernelGGL(aq_k_sum_parts, dim3((s->q_pad + 255) / 256), dim3(256), 0, 0, s->rnpart.get(), s->sums.get() + (size_t)4 * s->q_pad, s->laC, s->q_pad);
    if (a.dbg && s->it == 15) AQ_TRY(aq_diag_dump(dump, a.dbg, grid));
  } else {
    return aq_fail(AQ_ERR_UNSUPPORTED, "no core kernel selected for this problem");
  }
  AQ_HIP(hipEventRecord(e1, 0));
  AQ_HIP(hipGetLastError());
  if (mode == 0) {
    s->ev.push_back({e0, e1});
  } else {
    hipEventDestroy(e0);
    hipEventDestroy(e1);
  }
  return AQ_OK;
}

// part A of a sweep: S1-S11 + local reductions into the all-reduce payload
static int aq_launch_prepass(aq_vb *s, double c, int do_H) {
  AqPrepass &v = s->pre_args;
  v.sqrt_c = std::sqrt(c);
  v.c_is_one = aq_all_equal_1(c) ? 1 : 0;
  v.do_H = do_H;
  hipLaunchKernelGGL(aq_k_prepass, dim3(s->nHchunk, s->ntile), dim3(256), 0, 0, v);
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

static int aq_sweep_part_a(aq_vb *s) {
  if (!s->pre_done && !s->fused) AQ_TRY(aq_launch_prepass(s, s->c, 0));
  s->pre_done = false;
  hipLaunchKernelGGL(aq_k_qpre, dim3((s->q_pad + 255) / 256), dim3(256), 0, 0, s->qv, s->sc.get(), s->c);
  AQ_TRY(aq_launch_core(s, 0, s->c));
  hipLaunchKernelGGL(aq_k_reduce_rows, dim3((s->p_pad + 63) / 64), dim3(256), 0, 0, s->fused ? (const double *)nullptr : s->rowA.get(), s->rowGB.get(),
                     s->red, s->ntile, s->p_pad, s->WPT);
  hipLaunchKernelGGL(aq_k_reduce_q_scalars, dim3(1), dim3(1024), 0, 0, s->qv, s->red + s->p_pad);
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

// part B: S12-S20 on the all-reduced sums, then the ladder step (host scalars)
static int aq_sweep_part_b(aq_vb *s) {
  const AqQvec &qv = s->qv;
  const AqPvec &pv = s->pv;
  int ann = (s->annealing) ? 1 : 0;   // annealing & anneal_scale, :244
  hipLaunchKernelGGL(aq_k_take_reduced_scalars, dim3(1), dim3(1), 0, 0, s->sc.get(), s->red + s->p_pad);
  if (s->scheme == 1) {   // global-only core: R/atlasqtl_global_core.R:238-256
    hipLaunchKernelGGL(aq_k_pvec_global, dim3(s->pblk), dim3(256), 0, 0, pv, s->sc.get(), s->c, s->q_total);
    hipLaunchKernelGGL(aq_k_scalars_post_global, dim3(1), dim3(1024), 0, 0, pv, s->sc.get(), s->c_s, s->pblk);
  } else {
    hipLaunchKernelGGL(aq_k_reset_lentz, dim3(1), dim3(1), 0, 0, s->sc.get());
    hipLaunchKernelGGL(aq_k_pvec_L, dim3(s->pblk), dim3(256), 0, 0, pv, s->sc.get(), s->c_s, ann);
    hipLaunchKernelGGL(aq_k_pvec_finish, dim3(s->pblk), dim3(256), 0, 0, pv, s->sc.get(), s->c, s->c_s, ann, s->q_total);
    hipLaunchKernelGGL(aq_k_scalars_post, dim3(1), dim3(1024), 0, 0, pv, s->sc.get(), s->c_s, s->pblk);
  }
  hipLaunchKernelGGL(aq_k_qpost, dim3((s->q_pad + 255) / 256), dim3(256), 0, 0, qv, s->sc.get(), s->c, s->sig2_zeta, s->t02_inv);
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

static int aq_elbo_local(aq_vb *s) {
  const AqQvec &qv = s->qv;
  const AqPvec &pv = s->pv;
  // the pre-pass of the NEXT sweep (same refreshed theta + zeta, c = 1 here) also yields the p x q ELBO part
  AQ_TRY(aq_launch_prepass(s, s->c, 1));
  s->pre_done = !s->fused;
  if (s->scheme == 1) hipLaunchKernelGGL(aq_k_elbo_C_global, dim3(1), dim3(1), 0, 0, pv, s->sc.get());
  else hipLaunchKernelGGL(aq_k_elbo_C, dim3(1), dim3(1024), 0, 0, pv, s->sc.get());
  hipLaunchKernelGGL(aq_k_elbo_q, dim3(1), dim3(1024), 0, 0, qv, s->sc.get(), s->Hpart.get(), s->ntile * s->nHchunk, s->ered);
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

// Bounded waits inside the sweep kernels (a chained segment waiting for its predecessor, a sample part waiting for its
// partners' partial S) raise errflag when they expire: the results of that launch are invalid.  Polled wherever results
// leave the library: ELBO evaluation, end of a run, status, state and result getters.
int aq_check_chain_error(aq_vb *s) {
  if (!s->errflag.get() || (s->chain <= 1 && s->misC <= 1 && s->laC <= 1 && !s->errflag_forced)) return AQ_OK;
  int f = 0;
  AQ_HIP(hipMemcpy(&f, s->errflag.get(), sizeof(int), hipMemcpyDeviceToHost));
  if (f != 0) {
    s->failed = true;
    s->fail_code = AQ_ERR_DEVICE;
    s->fail_msg = (s->misC > 1 || s->laC > 1) ? "core sweep: a bounded wait on a partner workgroup's partial sums expired (results invalid)"
                              : "chained core sweep: a bounded wait on a tile's previous SNP segment expired (results invalid; set AQ_CHAIN=0)";
    return aq_fail(AQ_ERR_DEVICE, s->fail_msg);
  }
  return AQ_OK;
}

static int aq_elbo_finish(aq_vb *s, double *lb) {
  AqElboConst k;
  k.nu_h = s->nu; k.rho_h = s->rho; k.A2_inv = s->A2_inv; k.t02_inv = s->t02_inv;
  k.vec_sum_log_det_zeta = s->vec_sum_log_det_zeta; k.sig2_zeta = s->sig2_zeta;
  k.p = (double)s->p; k.q_total = (double)s->q_total;
  k.global_only = s->scheme == 1 ? 1 : 0;
  hipLaunchKernelGGL(aq_k_elbo_final, dim3(1), dim3(1), 0, 0, s->sc.get(), s->ered, k);
  AQ_HIP(hipGetLastError());
  AqScalars h;
  AQ_HIP(hipMemcpy(&h, s->sc.get(), sizeof(h), hipMemcpyDeviceToHost));
  AQ_TRY(aq_check_chain_error(s));
  *lb = h.elbo;
  return AQ_OK;
}

// One step of the state machine.  stop_after_sweeps < 0: unlimited.
static int aq_advance_impl(aq_vb *s, int *sweeps_budget) {
  if (s->failed) return -aq_fail(s->fail_code, "handle is in a failed state: " + s->fail_msg);
  AQ_HIP(hipSetDevice(s->device));
  for (;;) {
    switch (s->phase) {
      case 0: {   // initial residual R = Y - X beta_vb (:112-115 in n-space) and the initial column sums
        AQ_TRY(aq_launch_core(s, 1, 1.0));
        AQ_HIP(hipMemsetAsync(s->red, 0, (size_t)aq_vb_reduce_len(s->p) * sizeof(double), 0));
        hipLaunchKernelGGL(aq_k_reduce_q_scalars, dim3(1), dim3(1024), 0, 0, s->qv, s->red + s->p_pad);
        AQ_HIP(hipGetLastError());
        s->phase = 1;
        return AQ_VB_NEED_ALLREDUCE_MAIN;
      }
      case 1:
        hipLaunchKernelGGL(aq_k_take_reduced_scalars, dim3(1), dim3(1), 0, 0, s->sc.get(), s->red + s->p_pad);
        s->phase = 2;
        break;
      case 2:
        if (s->converged || s->it >= s->maxit) return AQ_VB_DONE;                  // :125
        if (sweeps_budget) {
          if (*sweeps_budget == 0) return AQ_VB_DONE;
          (*sweeps_budget)--;
        }
        s->lb_old = s->lb_new;                                                     // :127
        s->it += 1;
        AQ_TRY(aq_sweep_part_a(s));
        s->phase = 3;
        return AQ_VB_NEED_ALLREDUCE_MAIN;
      case 3: {
        AQ_TRY(aq_sweep_part_b(s));
        if (s->annealing) {                                                        // :318-337
          s->sig2_zeta = s->c * s->sig2_zeta;
          s->c = (s->it < (int)s->ladder.size()) ? s->ladder[s->it] : 1.0;         // ladder[it + 1], 1-based
          s->c_s = s->c;
          s->sig2_zeta = s->sig2_zeta / s->c;
          if (aq_all_equal_1(s->c)) s->annealing = false;
          s->phase = 2;
          break;
        }
        bool eval = (s->it <= s->it_init + 1) || (s->it % s->batch_conv == 0) || (s->it % s->batch_conv == 1);   // :342
        if (!eval) {
          s->phase = 2;
          break;
        }
        AQ_TRY(aq_elbo_local(s));
        s->phase = 4;
        return AQ_VB_NEED_ALLREDUCE_ELBO;
      }
      case 4: {
        double lb;
        AQ_TRY(aq_elbo_finish(s, &lb));
        s->lb_new = lb;
        s->trace_it.push_back(s->it);
        s->trace_lb.push_back(lb);
        const double eps = std::sqrt(std::numeric_limits<double>::epsilon());      // :85
        if (s->debug && lb + eps < s->lb_old) {                                    // :359-360
          s->failed = true;
          s->fail_code = AQ_ERR_NUMERIC;
          char buf[256];
          std::snprintf(buf, sizeof(buf), "ELBO not increasing monotonically. Exit. (it=%d, lb_old=%.17g, lb_new=%.17g)", s->it,
                        s->lb_old, lb);
          s->fail_msg = buf;
          return -aq_fail(AQ_ERR_NUMERIC, buf);
        }
        double diff = std::fabs(lb - s->lb_old);                                   // :362
        int sum_exceed = 0;
        for (double t : s->times_conv_sched) sum_exceed += (diff > t * s->tol) ? 1 : 0;   // :364
        if (sum_exceed == 0) {
          s->converged = true;
        } else if (s->ind_batch_conv > sum_exceed) {
          s->ind_batch_conv = sum_exceed;
          s->batch_conv = s->batch_conv_sched[sum_exceed - 1];
        }
        s->phase = 2;
        break;
      }
      default:
        return -aq_fail(AQ_ERR_ARG, "corrupt state");
    }
  }
}

extern "C" int aq_vb_advance(aq_vb_handle h) {
  if (!h) return -aq_fail(AQ_ERR_ARG, "NULL handle");
  int rc = aq_advance_impl(h, h->budget >= 0 ? &h->budget : nullptr);
  return rc;
}
extern "C" int aq_vb_set_sweep_budget(aq_vb_handle h, int32_t sweeps) {
  if (!h) return aq_fail(AQ_ERR_ARG, "NULL handle");
  h->budget = sweeps < 0 ? -1 : sweeps;
  return AQ_OK;
}

static int aq_run_impl(aq_vb *s, int *budget) {
  if (s->world != 1) return aq_fail(AQ_ERR_ARG, "aq_vb_run: world_size != 1 needs the aq_vb_advance protocol");
  for (;;) {
    int rc = aq_advance_impl(s, budget);
    if (rc < 0) return -rc;
    if (rc == AQ_VB_DONE) break;
  }
  AQ_HIP(hipDeviceSynchronize());
  return aq_check_chain_error(s);
}
extern "C" int aq_vb_run(aq_vb_handle h) {
  if (!h) return aq_fail(AQ_ERR_ARG, "NULL handle");
  return aq_run_impl(h, nullptr);
}
extern "C" int aq_vb_run_sweeps(aq_vb_handle h, int32_t max_sweeps) {
  if (!h) return aq_fail(AQ_ERR_ARG, "NULL handle");
  int budget = max_sweeps;
  return aq_run_impl(h, &budget);
}

void aq_resolve_events(aq_vb *s) {
  for (auto &e : s->ev) {
    float ms = 0.f;
    if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) {
      s->core_ms_acc += ms;
      s->core_launches++;
    }
    hipEventDestroy(e.first);
    hipEventDestroy(e.second);
  }
  s->ev.clear();
}
