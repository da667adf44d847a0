// aq_prep_marginal_perm.hip -- permutation nulls of the marginal screen of a finished prepare handle (include/atlasqtl_hip.h):
// aq_prep_marginal_perm evaluates the statistic of aq_prep_marginal on (Xs, Y') for every given permutation of the sample
// rows of Yc, a batch of permutations per launch (aq_msperm_kernels.h, planned by aq_msperm_plan.h), and returns per
// permutation each trait's largest r^2, the largest null hotspot size, the number of selected pairs and the number of
// undefined ones; aq_prep_marginal_perm_time times the kernels alone, aq_msperm_plan_query runs the planner on the host.  The
// kernels are plain HIP that issues no hand-written load: the ISA proof of the look-ahead sweep units does not cover them and
// need not.
#include "aq_screen_host.h"      // aq_screen_*; aq_prep.h, aq_internal.h; aq_screen_tile.h: aq_k_ms_gather, aq_k_ms_traitstats, aq_k_ms_colstats
#include "aq_msperm_kernels.h"   // aq_k_msperm_tile, aq_k_msperm_reduce; aq_msperm_make_plan, aq_msperm_check_rows

extern "C" int aq_msperm_plan_query(int32_t n, int32_t p1, int32_t q, int32_t masked, int32_t ncu, int32_t n_perm, aq_msperm_plan *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_msperm_plan_query: NULL argument");
  *out = aq_msperm_plan{};
  std::string err;
  const int rc = aq_msperm_make_plan(n, p1, q, masked, ncu, n_perm, 0, 0, 0, "aq_msperm_plan_query", out, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

// the device side of one call: what does not change with the permutation, and the buffers of one launch
struct AqMspBuf {
  AqDev<double> cut, sx, sxx, syy, Yp, max_r2;
  AqDev<int> mt;
  AqDev<int32_t> perm;
  AqDev<unsigned long long> key, undef;
  AqDev<unsigned int> count;
  AqDev<long long> hs, nsel;
  std::vector<int> mt_host;
  aq_msperm_plan pl{};
};

// Syy_t and m_t of the handle's traits (permutation-invariant), whether any value is missing, the plan, every buffer, and the
// complete instance's Sx and Sxx
static int aq_msp_setup(aq_prep *h, int n_perm, const char *who, AqMspBuf *b) {
  const size_t p1 = (size_t)h->p_kept, q = (size_t)h->q, n = (size_t)h->n;
  int masked = 0, ncu = 0;
  AQ_TRY(aq_screen_trait_stats(h, &b->syy, &b->mt, &b->mt_host, &masked, &ncu));
  std::string err;
  const int rc = aq_msperm_make_plan(h->n, h->p_kept, h->q, masked, ncu, n_perm, aq_screen_env("AQ_MSCREEN_TILE"),
                                     aq_screen_env("AQ_MSPERM_PB"), aq_screen_env("AQ_MSPERM_BATCH"), who, &b->pl, &err);
  if (rc != AQ_OK) return aq_fail(rc, err);
  const size_t batch = (size_t)b->pl.batch;
  AQ_TRY(b->cut.alloc(q));
  AQ_TRY(b->Yp.alloc(batch * q * n));
  AQ_TRY(b->perm.alloc(batch * n));
  AQ_TRY(b->key.alloc(batch * q));
  AQ_TRY(b->max_r2.alloc(batch * q));
  AQ_TRY(b->count.alloc(batch * p1));
  AQ_TRY(b->undef.alloc(batch));
  AQ_TRY(b->hs.alloc(batch));
  AQ_TRY(b->nsel.alloc(batch));
  if (!masked) {
    AQ_TRY(b->sx.alloc(p1));
    AQ_TRY(b->sxx.alloc(p1));
    hipLaunchKernelGGL(aq_k_ms_colstats, dim3((unsigned)p1), dim3(256), 0, 0, h->Xs.get(), h->n, b->sx.get(), b->sxx.get());
    AQ_HIP(hipGetLastError());
  }
  return AQ_OK;
}

template <int T, bool MASKED, int PB>
static void aq_msp_launch_tile(unsigned grid, const aq_msp_args &a) {
  aq_screen_a16(a.n, [&](auto a16) {   // even n: every column of Xs and of Yp starts at a multiple of 16 bytes
    hipLaunchKernelGGL((aq_k_msperm_tile<T, MASKED, decltype(a16)::value, PB>), dim3(grid), dim3(256), 0, 0, a);
  });
}

// the kernels of one launch over the nb <= batch permutations whose rows lie in b.perm, with b.cut holding the cutoffs.
// Asynchronous.
static int aq_msp_launch(aq_prep *h, AqMspBuf &b, int nb) {
  const int p1 = h->p_kept, q = h->q, n = h->n, pb = b.pl.pb;
  AQ_HIP(hipMemsetAsync(b.key.get(), 0, (size_t)nb * (size_t)q * sizeof(unsigned long long), 0));
  AQ_HIP(hipMemsetAsync(b.count.get(), 0, (size_t)nb * (size_t)p1 * sizeof(unsigned int), 0));
  AQ_HIP(hipMemsetAsync(b.undef.get(), 0, (size_t)nb * sizeof(unsigned long long), 0));
  const long long cols = (long long)nb * (long long)q;
  hipLaunchKernelGGL(aq_k_ms_gather, dim3((unsigned)(cols < (1ll << 20) ? cols : (1ll << 20))), dim3(256), 0, 0, h->Yc.get(),
                     (const int32_t *)nullptr, (const int32_t *)b.perm.get(), n, q, nb, b.Yp.get());
  aq_msp_args a{};
  a.Xs = h->Xs.get(); a.Yp = b.Yp.get();
  a.n = n; a.p1 = p1; a.q = q; a.n_cov = h->n_cov; a.tiles_p = b.pl.tiles_p;
  a.n_tiles = b.pl.tiles_p * b.pl.tiles_q;         // < 2^31, and so is the grid: the plan
  a.nb = nb;
  a.sx = b.sx.get(); a.sxx = b.sxx.get(); a.syy = b.syy.get(); a.mt = b.mt.get(); a.cut = b.cut.get();
  a.key = b.key.get(); a.count = b.count.get(); a.n_undef = b.undef.get();
  const unsigned grid = (unsigned)((long long)a.n_tiles * ((nb + pb - 1) / pb));
  if (b.pl.masked) {
    if (pb == 2)
      aq_msp_launch_tile<AQ_MSCREEN_TILE_MASKED, true, 2>(grid, a);
    else
      aq_msp_launch_tile<AQ_MSCREEN_TILE_MASKED, true, 1>(grid, a);
  } else if (b.pl.tile == 128) {
    aq_msp_launch_tile<128, false, 1>(grid, a);
  } else if (pb == 4) {
    aq_msp_launch_tile<64, false, 4>(grid, a);
  } else if (pb == 2) {
    aq_msp_launch_tile<64, false, 2>(grid, a);
  } else {
    aq_msp_launch_tile<64, false, 1>(grid, a);
  }
  hipLaunchKernelGGL(aq_k_msperm_reduce, dim3((unsigned)nb), dim3(256), 0, 0, b.count.get(), b.key.get(), p1, q, b.hs.get(), b.nsel.get(),
                     b.max_r2.get());
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

extern "C" int aq_prep_marginal_perm(aq_prep_handle h, const double *r2_cut, int32_t n_perm, const int32_t *perm, double *max_r2,
                                     int64_t *hs_max, int64_t *n_sel, int64_t *n_undef) {
  if (n_perm < 1) return aq_fail(AQ_ERR_ARG, "aq_prep_marginal_perm: n_perm >= 1 required, " + std::to_string(n_perm) + " given");
  if (!r2_cut || !perm) return aq_fail(AQ_ERR_ARG, "aq_prep_marginal_perm: NULL r2_cut or perm");
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_marginal_perm: NULL handle");
  AQ_TRY(aq_screen_need_cut(r2_cut, h->q, "aq_prep_marginal_perm"));
  {
    std::string err;                             // an index out of range never reaches the gather kernel
    const int rc = aq_msperm_check_rows(perm, n_perm, h->n, "aq_prep_marginal_perm", &err);
    if (rc != AQ_OK) return aq_fail(rc, err);
  }
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_marginal_perm"));
  const size_t q = (size_t)h->q, n = (size_t)h->n;
  AqMspBuf b;
  AQ_TRY(aq_msp_setup(h, n_perm, "aq_prep_marginal_perm", &b));
  AQ_HIP(hipMemcpy(b.cut.get(), r2_cut, q * sizeof(double), hipMemcpyHostToDevice));
  static_assert(sizeof(unsigned long long) == sizeof(int64_t) && sizeof(long long) == sizeof(int64_t), "the counts are copied as they are");
  for (int done = 0; done < n_perm; done += b.pl.batch) {
    const int nb = n_perm - done < b.pl.batch ? n_perm - done : b.pl.batch;
    AQ_HIP(hipMemcpy(b.perm.get(), perm + (size_t)done * n, (size_t)nb * n * sizeof(int32_t), hipMemcpyHostToDevice));
    AQ_TRY(aq_msp_launch(h, b, nb));
    if (max_r2) AQ_HIP(hipMemcpy(max_r2 + (size_t)done * q, b.max_r2.get(), (size_t)nb * q * sizeof(double), hipMemcpyDeviceToHost));
    if (hs_max) AQ_HIP(hipMemcpy(hs_max + done, b.hs.get(), (size_t)nb * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (n_sel) AQ_HIP(hipMemcpy(n_sel + done, b.nsel.get(), (size_t)nb * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (n_undef) AQ_HIP(hipMemcpy(n_undef + done, b.undef.get(), (size_t)nb * sizeof(int64_t), hipMemcpyDeviceToHost));
    AQ_HIP(hipDeviceSynchronize());              // the next launch overwrites the buffers
  }
  return AQ_OK;
}

// Timing hook of aq_prep_marginal_perm: the gather, tile and reduce kernels of n_perm permutations, launch by launch, `reps`
// times between two events, without the copies.  The rows are one batch of aq_screen_time_perms, used again by every launch;
// the cutoff is that of aq_prep_marginal_time.
extern "C" int aq_prep_marginal_perm_time(aq_prep_handle h, int32_t n_perm, int32_t reps, double *ms_per_perm, aq_msperm_plan *plan_out) {
  if (!h || !ms_per_perm) return aq_fail(AQ_ERR_ARG, "aq_prep_marginal_perm_time: NULL argument");
  if (n_perm < 1 || reps < 1) return aq_fail(AQ_ERR_ARG, "aq_prep_marginal_perm_time: n_perm >= 1 and reps >= 1 required");
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_marginal_perm_time"));
  const size_t q = (size_t)h->q, n = (size_t)h->n;
  AqMspBuf b;
  AQ_TRY(aq_msp_setup(h, n_perm, "aq_prep_marginal_perm_time", &b));
  if (plan_out) *plan_out = b.pl;
  std::vector<double> cut(q);
  for (size_t t = 0; t < q; t++) cut[t] = aq_screen_time_cut(b.mt_host[t] - 2 - h->n_cov);
  AQ_HIP(hipMemcpy(b.cut.get(), cut.data(), q * sizeof(double), hipMemcpyHostToDevice));
  const std::vector<int32_t> perm = aq_screen_time_perms((size_t)b.pl.batch, n);
  AQ_HIP(hipMemcpy(b.perm.get(), perm.data(), perm.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  double ms = 0.0;
  AQ_TRY(aq_time_launches(reps, &ms, [&] {
    for (int done = 0; done < n_perm; done += b.pl.batch)
      AQ_TRY(aq_msp_launch(h, b, n_perm - done < b.pl.batch ? n_perm - done : b.pl.batch));
    return (int)AQ_OK;
  }));
  *ms_per_perm = ms / (double)n_perm;
  return AQ_OK;
}
