// aq_vb_query.hip -- everything that reads a handle or post-processes its results: status, overrides, ELBO trace, result,
// residual, checkpoint / resume, and the post-processing and summary entries, both on a handle (aq_vb_*) and free-standing
// on host matrices.  Also the two conversions between column-major matrices and the trait-tiled layout, behind host functions.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "aq_vb.h"
#include "aq_layout_kernels.h"

int aq_tile_from_colmajor(const double *src, double *dst, int rows, int q, int rows_pad, int ntile, int nan_to_zero) {
  hipLaunchKernelGGL(aq_k_tile_from_colmajor, dim3((rows_pad + 63) / 64, ntile), dim3(256), 0, 0, src, dst, rows, q, rows_pad, nan_to_zero);
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}
int aq_colmajor_copy(const aq_vb *s, const double *src, const double *mul, int rows, int rows_pad, AqDev<double> *out) {
  AQ_TRY(out->alloc((size_t)rows * s->q));
  hipLaunchKernelGGL(aq_k_colmajor_from_tile, dim3((rows_pad + 63) / 64, s->ntile), dim3(256), 0, 0, src, mul, out->get(), rows, s->q, rows_pad);
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}
// as.vector(gam_vb): the p x q column-major copy that the full sort of assign_bFDR ranks
static int aq_gam_colmajor(const aq_vb *s, AqDev<double> *out) { return aq_colmajor_copy(s, s->gam.get(), nullptr, s->p, s->p_pad, out); }

extern "C" double *aq_vb_reduce_ptr(aq_vb_handle h, int32_t which) {
  if (!h) return nullptr;
  return which == 0 ? h->red : h->ered;
}

// ------------------------------------------------------------ post-processing ----
extern "C" int aq_assign_bfdr(const double *mat_ppi, double *mat_fdr, int64_t len, int32_t device) {
  if (!mat_ppi || !mat_fdr || len < 0) return aq_fail(AQ_ERR_ARG, "aq_assign_bfdr: bad argument");
  AQ_TRY(aq_need_device(device));
  if (len == 0) return AQ_OK;
  AqDev<double> din, dout;
  AQ_TRY(din.alloc((size_t)len));
  AQ_TRY(dout.alloc((size_t)len));
  AQ_HIP(hipMemcpy(din.get(), mat_ppi, (size_t)len * sizeof(double), hipMemcpyHostToDevice));
  AQ_TRY(aq_bfdr_device(din.get(), dout.get(), len));
  if (hipMemcpy(mat_fdr, dout.get(), (size_t)len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return aq_fail(AQ_ERR_DEVICE, "aq_assign_bfdr: copy back failed");
  return AQ_OK;
}

// d_m: p x q column-major PPIs on the device (overwritten by the FDR matrix when fdr_adjust)
static int aq_hotspot_common(double *d_m, int p, int q, double thres, int fdr_adjust, int64_t *rs_thres, int64_t *nb_pairwise) {
  int lt = 0;
  if (fdr_adjust) {
    AqDev<double> d_f;
    AQ_TRY(d_f.alloc((size_t)p * q));
    AQ_TRY(aq_bfdr_device(d_m, d_f.get(), (int64_t)p * q));
    if (hipMemcpy(d_m, d_f.get(), (size_t)p * q * sizeof(double), hipMemcpyDeviceToDevice) != hipSuccess)
      return aq_fail(AQ_ERR_DEVICE, "aq_hotspot_sizes: device copy failed");
    lt = 1;                                                      // rowSums(mat_fdr < thres), R/summarise_output.R:100
  }
  AqDev<int64_t> d_rs;
  AQ_TRY(d_rs.alloc((size_t)p));
  AQ_TRY(aq_row_count_device(d_m, d_rs.get(), p, q, thres, lt));    // rowSums(gam_vb > thres), :103
  std::vector<int64_t> rs(p);
  if (hipMemcpy(rs.data(), d_rs.get(), (size_t)p * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess)
    return aq_fail(AQ_ERR_DEVICE, "aq_hotspot_sizes: copy back failed");
  int64_t tot = 0;
  for (int j = 0; j < p; j++) { tot += rs[j]; if (rs_thres) rs_thres[j] = rs[j]; }
  if (nb_pairwise) *nb_pairwise = tot;                           // sum(gam_vb > thres), :102
  return AQ_OK;
}

extern "C" int aq_hotspot_sizes(const double *mat_ppi, int32_t p, int32_t q, double thres, int32_t fdr_adjust,
                                int64_t *rs_thres, int64_t *nb_pairwise, int32_t device) {
  if (!mat_ppi || p <= 0 || q <= 0) return aq_fail(AQ_ERR_ARG, "aq_hotspot_sizes: bad argument");
  AQ_TRY(aq_need_device(device));
  AqDev<double> d_m;
  AQ_TRY(d_m.alloc((size_t)p * q));
  AQ_HIP(hipMemcpy(d_m.get(), mat_ppi, (size_t)p * q * sizeof(double), hipMemcpyHostToDevice));
  return aq_hotspot_common(d_m.get(), p, q, thres, fdr_adjust, rs_thres, nb_pairwise);
}

extern "C" int aq_vb_hotspot_sizes(aq_vb_handle s, double thres, int32_t fdr_adjust, int64_t *rs_thres, int64_t *nb_pairwise) {
  if (!s) return aq_fail(AQ_ERR_ARG, "NULL handle");
  AQ_HIP(hipSetDevice(s->device));
  AqDev<double> d_m;
  AQ_TRY(aq_gam_colmajor(s, &d_m));
  return aq_hotspot_common(d_m.get(), s->p, s->q, thres, fdr_adjust, rs_thres, nb_pairwise);
}

// Bayesian FDR under trait sharding (aq_postproc.hip): the caller bisects over a PPI cutoff, all-reducing the five numbers
// of aq_vb_bfdr_query over the ranks at every step (atlasqtl_amd/core.py::VbRun.hotspot_sizes).
extern "C" int aq_vb_bfdr_begin(aq_vb_handle s) {
  if (!s) return aq_fail(AQ_ERR_ARG, "NULL handle");
  AQ_HIP(hipSetDevice(s->device));
  if (s->bf) { aq_shard_free(s->bf); s->bf = nullptr; }
  AqDev<double> d_m;
  AQ_TRY(aq_gam_colmajor(s, &d_m));
  return aq_shard_sort(d_m.get(), (int64_t)s->p * s->q, &s->bf);
}
extern "C" int aq_vb_bfdr_query(aq_vb_handle s, double c, double *out5) {
  if (!s || !out5 || !s->bf) return aq_fail(AQ_ERR_ARG, "aq_vb_bfdr_query: call aq_vb_bfdr_begin first");
  AQ_HIP(hipSetDevice(s->device));
  return aq_shard_query(s->bf, c, out5);
}
extern "C" int aq_vb_bfdr_rows(aq_vb_handle s, int64_t upto, int64_t tie_first, int64_t take, int64_t *rs) {
  if (!s || !rs || !s->bf) return aq_fail(AQ_ERR_ARG, "aq_vb_bfdr_rows: call aq_vb_bfdr_begin first");
  if (upto < 0 || take < 0 || tie_first < 0 || upto > (int64_t)s->p * s->q || tie_first + take > (int64_t)s->p * s->q)
    return aq_fail(AQ_ERR_ARG, "aq_vb_bfdr_rows: positions out of range");
  AQ_HIP(hipSetDevice(s->device));
  return aq_shard_rows(s->bf, upto, tie_first, take, s->p, rs);
}
extern "C" void aq_vb_bfdr_end(aq_vb_handle s) {
  if (s && s->bf) { hipSetDevice(s->device); aq_shard_free(s->bf); s->bf = nullptr; }
}

// Sparse table of associations (aq_postproc.hip): which (SNP, trait) pairs pass the threshold, with their effect sizes, in
// the order of order(as.vector(gam_vb), decreasing = TRUE) -- what summary.atlasqtl / plot.atlasqtl read off gam_vb
// (R/summarise_output.R:99-106) -- without a p x q matrix leaving the device.  Argument errors come before any device call.
static int aq_pairs_args(const char *who, bool ok, double thres, int64_t cap, const int64_t *n_pairs) {
  if (!ok || !n_pairs || thres != thres || cap < 0)
    return aq_fail(AQ_ERR_ARG, std::string(who) + ": bad argument (NULL handle / matrix / n_pairs, NaN thres or cap < 0)");
  return AQ_OK;
}
extern "C" int aq_vb_select_pairs(aq_vb_handle s, double thres, int32_t fdr_adjust, int64_t cap, int32_t *snp, int32_t *trait,
                                  double *ppi, double *beta, double *fdr, int64_t *n_pairs) {
  AQ_TRY(aq_pairs_args("aq_vb_select_pairs", s != nullptr, thres, cap, n_pairs));
  AQ_HIP(hipSetDevice(s->device));
  AQ_HIP(hipDeviceSynchronize());
  AQ_TRY(aq_check_chain_error(s));
  if (!fdr_adjust)     // reads the trait-tiled gam / mu where they are: nothing of size p q is allocated
    return aq_pairs_device(nullptr, s->gam.get(), s->mu.get(), s->p, s->q, s->p_pad, 1, thres, 0, cap, snp, trait, ppi, beta, fdr, n_pairs);
  AqDev<double> d_m;   // assign_bFDR ranks as.vector(gam_vb): the column-major copy aq_vb_hotspot_sizes makes as well
  AQ_TRY(aq_gam_colmajor(s, &d_m));
  return aq_pairs_device(d_m.get(), s->gam.get(), s->mu.get(), s->p, s->q, s->p_pad, 1, thres, 1, cap, snp, trait, ppi, beta, fdr, n_pairs);
}
extern "C" int aq_select_pairs(const double *mat_ppi, const double *mat_beta, int32_t p, int32_t q, double thres, int32_t fdr_adjust,
                               int64_t cap, int32_t *snp, int32_t *trait, double *ppi, double *beta, double *fdr, int64_t *n_pairs,
                               int32_t device) {
  AQ_TRY(aq_pairs_args("aq_select_pairs", mat_ppi != nullptr && p > 0 && q > 0, thres, cap, n_pairs));
  AQ_TRY(aq_need_device(device));
  const size_t pq = (size_t)p * q;
  AqDev<double> d_m, d_b;
  AQ_TRY(d_m.alloc(pq));
  AQ_HIP(hipMemcpy(d_m.get(), mat_ppi, pq * sizeof(double), hipMemcpyHostToDevice));
  if (mat_beta) {
    AQ_TRY(d_b.alloc(pq));
    AQ_HIP(hipMemcpy(d_b.get(), mat_beta, pq * sizeof(double), hipMemcpyHostToDevice));
  }
  return aq_pairs_device(d_m.get(), d_m.get(), d_b.get(), p, q, p, 0, thres, fdr_adjust, cap, snp, trait, ppi, beta, fdr, n_pairs);
}
extern "C" int aq_vb_bfdr_pairs(aq_vb_handle s, int64_t upto, int64_t tie_first, int64_t take, int32_t *snp, int32_t *trait,
                                double *ppi, double *beta) {
  if (!s || !s->bf) return aq_fail(AQ_ERR_ARG, "aq_vb_bfdr_pairs: call aq_vb_bfdr_begin first");
  if (upto < 0 || take < 0 || tie_first < 0 || upto > (int64_t)s->p * s->q || tie_first + take > (int64_t)s->p * s->q)
    return aq_fail(AQ_ERR_ARG, "aq_vb_bfdr_pairs: positions out of range");
  AQ_HIP(hipSetDevice(s->device));
  return aq_shard_pairs(s->bf, upto, tie_first, take, s->gam.get(), s->mu.get(), s->p, s->q, s->p_pad, snp, trait, ppi, beta);
}

// Order statistics and moments of gam_vb / beta_vb (aq_summary.hip): the six numbers of summary(as.vector(gam_vb)) and
// summary(as.vector(beta_vb)), R/summarise_output.R:89-93, from the trait-tiled state where it lies.  Argument errors come
// before any device call.
static int aq_ranks_args(const char *who, bool ok, int32_t n_ranks, const int64_t *ranks, const double *out) {
  bool good = ok && ranks && out && n_ranks >= 1 && n_ranks <= AQ_RSEL_MAX_PREFIX;
  for (int i = 0; good && i < n_ranks; i++) good = ranks[i] >= 0 && (i == 0 || ranks[i] >= ranks[i - 1]);
  if (!good)
    return aq_fail(AQ_ERR_ARG, std::string(who) + ": bad argument (NULL handle / array / ranks / out, which not 0 / 1, n_ranks "
                                                  "outside 1 ... 16, ranks negative or not ascending, or len < 1)");
  return AQ_OK;
}
static aq_pair_src aq_summary_src(const aq_vb *s, int which) {
  return aq_pair_src{s->gam.get(), which ? s->mu.get() : nullptr, s->p, s->q, s->p_pad, 1};
}
// results are about to leave the library: wait for the sweeps and poll the bounded-wait flag, as aq_vb_get_result does
static int aq_summary_ready(aq_vb *s) {
  AQ_HIP(hipSetDevice(s->device));
  AQ_HIP(hipDeviceSynchronize());
  return aq_check_chain_error(s);
}
extern "C" int aq_vb_radix_hist(aq_vb_handle s, int32_t which, int32_t n_prefix, const uint64_t *prefix, int32_t shift,
                                int64_t *hist) {
  const bool top = shift + AQ_RSEL_BITS == 64;
  bool good = s && hist && (which == 0 || which == 1) && shift >= 0 && shift < 64 && shift % AQ_RSEL_BITS == 0 && n_prefix >= 1 &&
              n_prefix <= (top ? 1 : AQ_RSEL_MAX_PREFIX) && (top || prefix);
  for (int i = 1; good && !top && i < n_prefix; i++) good = prefix[i] > prefix[i - 1];
  if (!good)
    return aq_fail(AQ_ERR_ARG, "aq_vb_radix_hist: bad argument (NULL handle / prefix / hist, which not 0 / 1, shift not a multiple of "
                               "AQ_RSEL_BITS in [0, 64), n_prefix outside 1 ... 16 (1 at the top digit), or prefixes not ascending)");
  AQ_TRY(aq_summary_ready(s));
  const aq_pair_src src = aq_summary_src(s, which);
  return aq_rsel_hist_device(src, aq_src_elements(src, 0), n_prefix, prefix, shift, hist);
}
extern "C" int aq_vb_moments(aq_vb_handle s, int32_t which, aq_moments *out) {
  if (!s || !out || (which != 0 && which != 1))
    return aq_fail(AQ_ERR_ARG, "aq_vb_moments: bad argument (NULL handle / out, or which not 0 / 1)");
  AQ_TRY(aq_summary_ready(s));
  const aq_pair_src src = aq_summary_src(s, which);
  return aq_moments_device(src, aq_src_elements(src, 0), out);
}
extern "C" int aq_vb_order_stats(aq_vb_handle s, int32_t which, int32_t n_ranks, const int64_t *ranks, double *out, aq_moments *mom) {
  AQ_TRY(aq_ranks_args("aq_vb_order_stats", s != nullptr && (which == 0 || which == 1), n_ranks, ranks, out));
  AQ_TRY(aq_summary_ready(s));
  const aq_pair_src src = aq_summary_src(s, which);
  return aq_order_stats_device(src, aq_src_elements(src, 0), n_ranks, ranks, out, mom, "aq_vb_order_stats");
}
extern "C" int aq_order_stats(const double *x, int64_t len, int32_t n_ranks, const int64_t *ranks, double *out, aq_moments *mom,
                              int32_t device) {
  AQ_TRY(aq_ranks_args("aq_order_stats", x != nullptr && len >= 1, n_ranks, ranks, out));
  AQ_TRY(aq_need_device(device));
  AqDev<double> d_x;
  AQ_TRY(d_x.alloc((size_t)len));
  AQ_HIP(hipMemcpy(d_x.get(), x, (size_t)len * sizeof(double), hipMemcpyHostToDevice));
  const aq_pair_src src{d_x.get(), nullptr, 0, 0, 0, 0};
  return aq_order_stats_device(src, (size_t)len, n_ranks, ranks, out, mom, "aq_order_stats");
}

// ------------------------------------------------------ checkpoint / resume ----
// The reference's checkpoint_ (R/utils.R:571-611) only writes outputs; it cannot resume.  Here the complete loop state
// between two sweeps is one flat blob: header, host-side loop scalars, ELBO trace, then the device arrays the next
// sweep reads (gam, mu, the incrementally updated residual, p- and q-vectors, column sums, AqScalars).  A, b and the row
// sums of the pre-pass are not stored: the next sweep recomputes them from theta and zeta (same kernel, same bits).
struct AqStateHeader {
  uint64_t magic;        // "AQVBST02"
  int32_t n, p, q, q_total, p_pad, q_pad, n_pad, core_kernel;
  int32_t it, converged, annealing, ind_batch_conv, batch_conv, failed, n_trace, has_missing;
  int32_t trait_offset, scheme_df;  // which trait shard of a q-sharded run the state belongs to; scheme + 16 df
  double c, c_s, sig2_zeta, lb_new, lb_old;
};
static const uint64_t AQ_STATE_MAGIC = 0x32305453425651ull | ((uint64_t)'A' << 56);

struct AqStateSeg { void *ptr; size_t bytes; };
static std::vector<AqStateSeg> aq_state_segments(aq_vb *s) {
  const size_t pq = (size_t)s->ntile * s->p_pad * 16 * sizeof(double);
  const size_t P = (size_t)s->p_pad * sizeof(double), Q = (size_t)s->q_pad * sizeof(double);
  std::vector<AqStateSeg> v = {
      {s->gam.get(), pq}, {s->mu.get(), pq}, {s->R.get(), (size_t)s->ntile * s->n_pad * 16 * sizeof(double)},
      {s->theta.get(), P}, {s->sig2_theta.get(), P}, {s->L.get(), P}, {s->lam2_inv.get(), P}, {s->Q.get(), P},
      {s->zeta.get(), Q}, {s->tau.get(), Q}, {s->sig2b.get(), Q}, {s->log_tau.get(), Q}, {s->eta_vb.get(), Q}, {s->kappa_vb.get(), Q},
      {s->coef.get(), Q}, {s->inv2s.get(), Q}, {s->cst.get(), Q}, {s->sums.get(), 6 * Q}, {s->sc.get(), sizeof(AqScalars)}};
  return v;
}
extern "C" int64_t aq_vb_state_bytes(aq_vb_handle s) {
  if (!s) return -1;
  size_t tot = sizeof(AqStateHeader) + s->trace_it.size() * (sizeof(int32_t) + sizeof(double));
  for (auto &g : aq_state_segments(s)) tot += g.bytes;
  return (int64_t)tot;
}

extern "C" int aq_vb_get_state(aq_vb_handle s, void *buf, int64_t cap) {
  if (!s || !buf) return aq_fail(AQ_ERR_ARG, "NULL argument");
  if (s->phase != 2) return aq_fail(AQ_ERR_ARG, "aq_vb_get_state: only between sweeps (after aq_vb_run / aq_vb_run_sweeps returned)");
  if (cap < aq_vb_state_bytes(s)) return aq_fail(AQ_ERR_ARG, "aq_vb_get_state: buffer too small");
  AQ_HIP(hipSetDevice(s->device));
  AQ_HIP(hipDeviceSynchronize());
  AQ_TRY(aq_check_chain_error(s));
  AqStateHeader h;
  std::memset(&h, 0, sizeof(h));
  h.magic = AQ_STATE_MAGIC;
  h.n = s->n; h.p = s->p; h.q = s->q; h.q_total = s->q_total; h.p_pad = s->p_pad; h.q_pad = s->q_pad; h.n_pad = s->n_pad;
  h.core_kernel = aq_core_kernel_id(*s); h.trait_offset = s->trait_offset; h.scheme_df = s->scheme + 16 * s->df;
  h.it = s->it; h.converged = s->converged; h.annealing = s->annealing; h.ind_batch_conv = s->ind_batch_conv;
  h.batch_conv = s->batch_conv; h.failed = s->failed; h.n_trace = (int32_t)s->trace_it.size(); h.has_missing = s->has_missing;
  h.c = s->c; h.c_s = s->c_s; h.sig2_zeta = s->sig2_zeta; h.lb_new = s->lb_new; h.lb_old = s->lb_old;
  char *o = (char *)buf;
  std::memcpy(o, &h, sizeof(h)); o += sizeof(h);
  for (int i = 0; i < h.n_trace; i++) { int32_t v = s->trace_it[i]; std::memcpy(o, &v, sizeof(v)); o += sizeof(v); }
  for (int i = 0; i < h.n_trace; i++) { double v = s->trace_lb[i]; std::memcpy(o, &v, sizeof(v)); o += sizeof(v); }
  for (auto &g : aq_state_segments(s)) {
    AQ_HIP(hipMemcpy(o, g.ptr, g.bytes, hipMemcpyDeviceToHost));
    o += g.bytes;
  }
  return AQ_OK;
}

extern "C" int aq_vb_set_state(aq_vb_handle s, const void *buf, int64_t len) {
  if (!s || !buf) return aq_fail(AQ_ERR_ARG, "NULL argument");
  if (len < (int64_t)sizeof(AqStateHeader)) return aq_fail(AQ_ERR_ARG, "aq_vb_set_state: truncated state");
  AqStateHeader h;
  const char *o = (const char *)buf;
  std::memcpy(&h, o, sizeof(h)); o += sizeof(h);
  if (h.magic != AQ_STATE_MAGIC) return aq_fail(AQ_ERR_ARG, "aq_vb_set_state: not an atlasqtl-hip state blob");
  if (h.n != s->n || h.p != s->p || h.q != s->q || h.q_total != s->q_total || h.has_missing != (int)s->has_missing)
    return aq_fail(AQ_ERR_ARG, "aq_vb_set_state: the state was saved for a different problem shape");
  if (h.core_kernel != aq_core_kernel_id(*s))
    return aq_fail(AQ_ERR_ARG, "aq_vb_set_state: the state was saved by core kernel " + std::to_string(h.core_kernel) + ", this handle runs kernel " +
                                   std::to_string(aq_core_kernel_id(*s)) + " (0 look-ahead MFMA, 2 generic, 3 masked two-barrier): create the handle with AQ_KERNEL / "
                                   "AQ_GK_MAX_GB set as for the run that saved it");
  if (h.p_pad != s->p_pad || h.q_pad != s->q_pad || h.n_pad != s->n_pad)
    return aq_fail(AQ_ERR_ARG, "aq_vb_set_state: same problem, different kernel geometry (padding " + std::to_string(h.n_pad) + " / " + std::to_string(h.q_pad) +
                                   " saved, " + std::to_string(s->n_pad) + " / " + std::to_string(s->q_pad) + " here): the launch plan depends on the "
                                   "device's CU count and on AQ_TT / AQ_LA_C / AQ_NT3; resume with the settings of the run that saved the state");
  if (h.trait_offset != s->trait_offset)
    return aq_fail(AQ_ERR_ARG, "aq_vb_set_state: the state belongs to another trait shard (trait_offset differs)");
  if (h.scheme_df != s->scheme + 16 * s->df)
    return aq_fail(AQ_ERR_ARG, "aq_vb_set_state: the state was saved under another scheme (global-local / global-only) or df");
  size_t need = sizeof(h) + (size_t)h.n_trace * (sizeof(int32_t) + sizeof(double));
  for (auto &g : aq_state_segments(s)) need += g.bytes;
  if (h.n_trace < 0 || (int64_t)need != len) return aq_fail(AQ_ERR_ARG, "aq_vb_set_state: state size mismatch");
  AQ_HIP(hipSetDevice(s->device));
  AQ_HIP(hipDeviceSynchronize());
  s->trace_it.resize(h.n_trace);
  s->trace_lb.resize(h.n_trace);
  for (int i = 0; i < h.n_trace; i++) { int32_t v; std::memcpy(&v, o, sizeof(v)); o += sizeof(v); s->trace_it[i] = v; }
  for (int i = 0; i < h.n_trace; i++) { double v; std::memcpy(&v, o, sizeof(v)); o += sizeof(v); s->trace_lb[i] = v; }
  for (auto &g : aq_state_segments(s)) {
    AQ_HIP(hipMemcpy(g.ptr, o, g.bytes, hipMemcpyHostToDevice));
    o += g.bytes;
  }
  s->it = h.it; s->converged = h.converged != 0; s->annealing = h.annealing != 0; s->ind_batch_conv = h.ind_batch_conv;
  s->batch_conv = h.batch_conv; s->failed = h.failed != 0;
  s->c = h.c; s->c_s = h.c_s; s->sig2_zeta = h.sig2_zeta; s->lb_new = h.lb_new; s->lb_old = h.lb_old;
  s->pre_done = false;   // the next sweep recomputes the pre-pass from the restored theta / zeta
  s->phase = 2;
  return AQ_OK;
}

extern "C" int aq_vb_get_status(aq_vb_handle s, aq_vb_status *st) {
  if (!s || !st) return aq_fail(AQ_ERR_ARG, "NULL argument");
  AQ_HIP(hipSetDevice(s->device));
  aq_resolve_events(s);
  AQ_TRY(aq_check_chain_error(s));
  AqScalars h;
  AQ_HIP(hipMemcpy(&h, s->sc.get(), sizeof(h), hipMemcpyDeviceToHost));
  st->it = s->it;
  st->converged = s->converged ? 1 : 0;
  st->lb_opt = s->lb_new;
  st->diff_lb = std::fabs(s->lb_new - s->lb_old);
  st->c = s->c;
  st->annealing = s->annealing ? 1 : 0;
  st->n_elbo = (int)s->trace_it.size();
  st->core_ms = s->core_ms_acc;
  st->core_launches = s->core_launches;
  st->sig02_inv_vb = h.sig02_inv;
  st->sig2_inv_vb = h.sig2_inv;
  st->lentz_iters = h.lentz_iters;
  aq_plan_to_status(*s, st);
  return AQ_OK;
}

extern "C" int32_t aq_vb_get_overrides(aq_vb_handle s, char *buf, int32_t cap) {
  if (!s) return -1;
  const int32_t n = (int32_t)s->overrides.size();
  if (buf && cap > 0) {
    const int32_t m = n < cap - 1 ? n : cap - 1;
    std::memcpy(buf, s->overrides.data(), (size_t)m);
    buf[m] = 0;
  }
  return n;
}

extern "C" int32_t aq_vb_get_elbo_trace(aq_vb_handle s, int32_t *it_out, double *lb_out, int32_t cap) {
  if (!s) return 0;
  int n = (int)s->trace_it.size();
  for (int i = 0; i < n && i < cap; i++) {
    if (it_out) it_out[i] = s->trace_it[i];
    if (lb_out) lb_out[i] = s->trace_lb[i];
  }
  return n;
}

extern "C" int aq_vb_get_result(aq_vb_handle s, double *beta_vb, double *gam_vb, double *mu_beta_vb, double *theta_vb,
                                double *zeta_vb, double *lam2_inv_vb, double *sig2_theta_vb, double *tau_vb,
                                double *sig2_beta_vb) {
  if (!s) return aq_fail(AQ_ERR_ARG, "NULL handle");
  AQ_HIP(hipSetDevice(s->device));
  AQ_HIP(hipDeviceSynchronize());
  AQ_TRY(aq_check_chain_error(s));
  size_t pq = (size_t)s->p * s->q;
  if (beta_vb || gam_vb || mu_beta_vb) {
    struct { double *dst; const double *src; const double *mul; } jobs[3] = {
        {beta_vb, s->gam.get(), s->mu.get()}, {gam_vb, s->gam.get(), nullptr}, {mu_beta_vb, s->mu.get(), nullptr}};
    for (auto &j : jobs) {
      if (!j.dst) continue;
      AqDev<double> stage;
      AQ_TRY(aq_colmajor_copy(s, j.src, j.mul, s->p, s->p_pad, &stage));
      AQ_HIP(hipMemcpy(j.dst, stage.get(), pq * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  if (theta_vb) AQ_HIP(hipMemcpy(theta_vb, s->theta.get(), (size_t)s->p * sizeof(double), hipMemcpyDeviceToHost));
  if (zeta_vb) AQ_HIP(hipMemcpy(zeta_vb, s->zeta.get(), (size_t)s->q * sizeof(double), hipMemcpyDeviceToHost));
  if (lam2_inv_vb) AQ_HIP(hipMemcpy(lam2_inv_vb, s->lam2_inv.get(), (size_t)s->p * sizeof(double), hipMemcpyDeviceToHost));
  if (sig2_theta_vb) AQ_HIP(hipMemcpy(sig2_theta_vb, s->sig2_theta.get(), (size_t)s->p * sizeof(double), hipMemcpyDeviceToHost));
  if (tau_vb) AQ_HIP(hipMemcpy(tau_vb, s->tau.get(), (size_t)s->q * sizeof(double), hipMemcpyDeviceToHost));
  if (sig2_beta_vb) AQ_HIP(hipMemcpy(sig2_beta_vb, s->sig2b.get(), (size_t)s->q * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}

// The residual the sweep kernel carries in n-space, mis_pat .* (Y - X beta_vb) (= what cp_Y_X - cp_betaX_X of the reference
// encodes, src/coreLoop.cpp:71,81), n x q column-major.  It is only ever updated incrementally (R -= X delta per SNP block and
// sweep), so comparing it with Y - X beta_vb recomputed from the returned beta_vb measures the rounding drift of a whole run.
extern "C" int aq_vb_get_residual(aq_vb_handle s, double *R_out) {
  if (!s || !R_out) return aq_fail(AQ_ERR_ARG, "NULL argument");
  AQ_HIP(hipSetDevice(s->device));
  AQ_HIP(hipDeviceSynchronize());
  AQ_TRY(aq_check_chain_error(s));
  if (s->use_tw && s->WPT > 1) return aq_fail(AQ_ERR_UNSUPPORTED, "aq_vb_get_residual: not for the generic kernel's split layout");
  const size_t nq = (size_t)s->n * s->q;
  AqDev<double> stage;
  AQ_TRY(aq_colmajor_copy(s, s->R.get(), nullptr, s->n, s->n_pad, &stage));
  AQ_HIP(hipMemcpy(R_out, stage.get(), nq * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}
