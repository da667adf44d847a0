// aq_prep_ld.hip -- LD pruning of a finished prepare handle (include/atlasqtl_hip.h, aq_prep_ld_prune; kernels in
// aq_ld_kernels.h): the banded correlation matrix of the compact matrix on the f64 matrix pipe, thresholded into bits, a
// first-one-wins scan, the r^2 of every removed column with its tag and a gather of the kept columns; aq_prep_ld_info reports
// what was removed, aq_prep_ld_band returns the band itself.  The kernels are plain HIP that issues no hand-written load: the
// ISA proof of the look-ahead sweep units does not cover them and need not.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "aq_prep.h"          // aq_prep; aq_internal.h: aq_fail, AQ_HIP, aq_need_device, aq_need_acc_layout, AqDev
#include "aq_ld_kernels.h"    // aq_k_ld_band, aq_k_ld_scan, aq_k_ld_tag_r2, aq_k_ld_gather

static int aq_ld_check_window(int32_t window, const char *who) {
  if (window < 1 || window > AQ_LD_MAX_WINDOW)
    return aq_fail(AQ_ERR_ARG, std::string(who) + ": window must lie in [1, " + std::to_string(AQ_LD_MAX_WINDOW) + "], " +
                                   std::to_string(window) + " given");
  return AQ_OK;
}

static dim3 aq_ld_grid(int p1, int window) { return dim3((unsigned)((p1 + 63) / 64), (unsigned)((window + 63) / 64)); }

extern "C" int aq_prep_ld_prune(aq_prep_handle h, const aq_prep_ld *ld) {
  if (!ld) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_prune: NULL argument");
  AQ_TRY(aq_ld_check_window(ld->window, "aq_prep_ld_prune"));
  if (!(ld->r2 > 0.0 && ld->r2 <= 1.0))
    return aq_fail(AQ_ERR_ARG, "aq_prep_ld_prune: r2 must lie in (0, 1], " + std::to_string(ld->r2) + " given");
  if (ld->window_bp > 0 && !ld->pos)
    return aq_fail(AQ_ERR_ARG, "aq_prep_ld_prune: window_bp = " + std::to_string(ld->window_bp) + " needs the positions (pos is NULL)");
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_prune: NULL handle");
  if (h->ld_done) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_prune: the handle has been pruned already (once per handle)");
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_ld_prune"));
  const int n = h->n, p = h->p, p1 = h->p_kept, window = ld->window, nw = (window + 63) / 64;
  const bool with_pos = ld->window_bp > 0;
  std::vector<int32_t> orig;                   // compact index -> original column
  orig.reserve((size_t)p1);
  for (int j = 0; j < p; j++)
    if (!h->bool_cst[j] && !h->bool_coll[j]) orig.push_back(j);
  AqDev<int32_t> dgroup, dof, ddst;
  AqDev<long long> dpos;
  AqDev<unsigned long long> dbits;
  AqDev<uint8_t> dbool;
  AqDev<double> dr2, Xnew;
  if (ld->group) {
    std::vector<int32_t> cg((size_t)p1);
    for (int c = 0; c < p1; c++) cg[c] = ld->group[orig[c]];
    AQ_TRY(dgroup.alloc((size_t)p1));
    AQ_HIP(hipMemcpy(dgroup.get(), cg.data(), cg.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  if (with_pos) {
    std::vector<long long> cp((size_t)p1);
    for (int c = 0; c < p1; c++) cp[c] = (long long)ld->pos[orig[c]];
    AQ_TRY(dpos.alloc((size_t)p1));
    AQ_HIP(hipMemcpy(dpos.get(), cp.data(), cp.size() * sizeof(long long), hipMemcpyHostToDevice));
  }
  AQ_TRY(dbits.alloc((size_t)p1 * nw));
  AQ_TRY(dbool.alloc((size_t)p1));
  AQ_TRY(dof.alloc((size_t)p1));
  AQ_TRY(dr2.alloc((size_t)p1));
  hipLaunchKernelGGL((aq_k_ld_band<true>), aq_ld_grid(p1, window), dim3(256), 0, 0, h->Xs.get(), n, p1, window, ld->r2, dgroup.get(),
                     dpos.get(), with_pos ? (long long)ld->window_bp : 0ll, (double *)nullptr, dbits.get(), nw);
  hipLaunchKernelGGL(aq_k_ld_scan, dim3(1), dim3(64), 0, 0, dbits.get(), p1, nw, dbool.get(), dof.get());
  hipLaunchKernelGGL(aq_k_ld_tag_r2, dim3(p1), dim3(256), 0, 0, h->Xs.get(), n, dof.get(), dr2.get());
  AQ_HIP(hipGetLastError());
  std::vector<uint8_t> rm((size_t)p1);
  std::vector<int32_t> of((size_t)p1), dst((size_t)p1, -1);
  std::vector<double> r2((size_t)p1);
  AQ_HIP(hipMemcpy(rm.data(), dbool.get(), rm.size(), hipMemcpyDeviceToHost));
  AQ_HIP(hipMemcpy(of.data(), dof.get(), of.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  AQ_HIP(hipMemcpy(r2.data(), dr2.get(), r2.size() * sizeof(double), hipMemcpyDeviceToHost));
  int p2 = 0;
  for (int c = 0; c < p1; c++)
    if (!rm[c]) dst[c] = p2++;
  if (p2 < p1) {                               // gather the kept columns, then release the matrix they came from
    AQ_TRY(ddst.alloc((size_t)p1));
    AQ_HIP(hipMemcpy(ddst.get(), dst.data(), dst.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    AQ_TRY(Xnew.alloc((size_t)n * p2));
    hipLaunchKernelGGL(aq_k_ld_gather, dim3(p1), dim3(256), 0, 0, h->Xs.get(), n, ddst.get(), Xnew.get());
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipDeviceSynchronize());
    h->Xs = std::move(Xnew);
  }
  h->ld_removed.assign((size_t)p, 0);
  h->ld_of.assign((size_t)p, -1);
  h->ld_r2.assign((size_t)p, std::nan(""));
  for (int c = 0; c < p1; c++)
    if (rm[c]) {
      h->ld_removed[orig[c]] = 1;
      h->ld_of[orig[c]] = orig[of[c]];
      h->ld_r2[orig[c]] = r2[c];
    }
  h->p_kept = p2;
  h->ld_done = true;
  return AQ_OK;
}

extern "C" int aq_prep_ld_info(aq_prep_handle h, int32_t *p_kept, uint8_t *bool_ld, int32_t *ld_of, double *ld_r2) {
  if (!h) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_info: NULL handle");
  if (!h->ld_done) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_info: aq_prep_ld_prune has not run on the handle");
  if (p_kept) *p_kept = h->p_kept;
  if (bool_ld) std::copy(h->ld_removed.begin(), h->ld_removed.end(), bool_ld);
  if (ld_of) std::copy(h->ld_of.begin(), h->ld_of.end(), ld_of);
  if (ld_r2) std::copy(h->ld_r2.begin(), h->ld_r2.end(), ld_r2);
  return AQ_OK;
}

extern "C" int aq_prep_ld_band(aq_prep_handle h, int32_t window, double *r_band) {
  AQ_TRY(aq_ld_check_window(window, "aq_prep_ld_band"));
  if (!h || !r_band) return aq_fail(AQ_ERR_ARG, "aq_prep_ld_band: NULL argument");
  AQ_TRY(aq_need_device(h->device));
  AQ_TRY(aq_need_acc_layout("aq_prep_ld_band"));
  const int p1 = h->p_kept;
  const size_t len = (size_t)p1 * window;
  AqDev<double> dband;
  AQ_TRY(dband.alloc(len));
  hipLaunchKernelGGL((aq_k_ld_band<false>), aq_ld_grid(p1, window), dim3(256), 0, 0, h->Xs.get(), h->n, p1, window, 1.0,
                     (const int32_t *)nullptr, (const long long *)nullptr, 0ll, dband.get(), (unsigned long long *)nullptr, 0);
  AQ_HIP(hipGetLastError());
  AQ_HIP(hipMemcpy(r_band, dband.get(), len * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}
