// aq_ciscond_plan.h -- the launch plan of the conditional cis scan (aq_prep_cis_cond; kernels in aq_ciscond_kernels.h): the
// plan of aq_cis_plan.h for the same windows (complete Y, no permutations: the order of the traits, the trait tiles and the
// work items are taken over unchanged), and on top of it what the conditioning lists decide: KC, the instance of the tile
// kernel, which is the smallest of 1, 2, 4 that holds the longest list of a trait WITH a window (0: no such trait has a list,
// and the plain tile kernel of aq_cis_kernels.h runs); the static LDS of that instance; the bytes of the basis panels Qo
// [KC][q_active][n] and of the residual traits Yo [q_active][n].  A pure function in the manner of aq_cis_plan.h: integer
// arithmetic only, no HIP call, no getenv.  aq_prep_cis_cond runs it before it allocates anything; aq_ciscond_plan_query
// exposes it on the C ABI without a device.  The check of the conditioning lists is here too: it is host arithmetic.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "aq_cis_plan.h"

#define AQ_CISCOND_KMAX 4                    // conditioning variants per trait
#define AQ_CISCOND_PANEL_MAX (4ll << 30)     // bytes of Qo and Yo together

AQ_MSCREEN_HD constexpr bool aq_ciscond_instance(int kc) { return kc == 1 || kc == 2 || kc == 4; }

// the smallest instance that holds k conditioning variants; 0 for k = 0
AQ_MSCREEN_HD constexpr int aq_ciscond_kc(int k) { return k <= 0 ? 0 : k == 1 ? 1 : k == 2 ? 2 : 4; }

// static LDS of a workgroup of aq_k_cc_tile<KC, ...>: the panel of X and the 1 + KC trait-side panels (the residual traits, the
// KC basis vectors), rows of AQ_MSCREEN_STR doubles; the two columns of per-trait candidates (double r, int snp); per trait
// S~yy_t, the cutoff, whether the trait can be tested, s_lo, s_hi and the trait's own index.  KC = 0: the plain scan's.
AQ_MSCREEN_HD constexpr int aq_ciscond_lds_bytes(int kc) {
  return kc == 0 ? aq_cis_lds_bytes(false)
                 : (2 + kc) * AQ_CIS_TILE * AQ_MSCREEN_STR * 8 + 2 * AQ_CIS_TILE * (8 + 4) + AQ_CIS_TILE * (8 + 8 + 4 + 4 + 4 + 4);
}

// cond_ptr: q + 1 offsets, non-decreasing from 0; trait t conditions on cond_idx[cond_ptr[t]] ... cond_idx[cond_ptr[t + 1] - 1]:
// at most AQ_CISCOND_KMAX distinct indices in [0, p1).  cond_idx may be NULL when the lists are only counted (the query) or
// when every list is empty.  too_many: what a list longer than AQ_CISCOND_KMAX returns (AQ_ERR_ARG from the entry,
// AQ_ERR_UNSUPPORTED from the planner).
static inline int aq_ciscond_check_lists(const int32_t *cond_ptr, const int32_t *cond_idx, int q, int p1, int too_many, const char *who,
                                         std::string *err) {
  const std::string w(who);
  if (!cond_ptr) {
    if (err) *err = w + ": NULL cond_ptr";
    return AQ_ERR_ARG;
  }
  if (cond_ptr[0] != 0) {
    if (err) *err = w + ": cond_ptr[0] must be 0, " + std::to_string(cond_ptr[0]) + " given";
    return AQ_ERR_ARG;
  }
  for (int t = 0; t < q; t++)
    if (cond_ptr[t + 1] < cond_ptr[t]) {
      if (err) *err = w + ": cond_ptr decreases at trait " + std::to_string(t);
      return AQ_ERR_ARG;
    }
  for (int t = 0; t < q; t++) {
    const int k = cond_ptr[t + 1] - cond_ptr[t];
    if (k > AQ_CISCOND_KMAX) {
      if (err)
        *err = w + ": trait " + std::to_string(t) + " conditions on " + std::to_string(k) + " variants, at most " +
               std::to_string(AQ_CISCOND_KMAX) + " are supported";
      return too_many;
    }
  }
  if (!cond_idx) {
    if (cond_ptr[q] > 0 && too_many == AQ_ERR_ARG) {
      if (err) *err = w + ": NULL cond_idx";
      return AQ_ERR_ARG;
    }
    return AQ_OK;
  }
  for (int t = 0; t < q; t++)
    for (int a = cond_ptr[t]; a < cond_ptr[t + 1]; a++) {
      const long long c = cond_idx[a];
      if (c < 0 || c >= p1) {
        if (err)
          *err = w + ": conditioning index " + std::to_string(c) + " of trait " + std::to_string(t) + " is outside [0, " +
                 std::to_string(p1) + ")";
        return AQ_ERR_ARG;
      }
      for (int b = cond_ptr[t]; b < a; b++)
        if (cond_idx[b] == cond_idx[a]) {
          if (err) *err = w + ": trait " + std::to_string(t) + " conditions on predictor " + std::to_string(c) + " more than once";
          return AQ_ERR_ARG;
        }
    }
  return AQ_OK;
}

// work may be NULL (the query).  The windows and the lists are checked again here, so that the query refuses what the entry
// refuses.
static inline int aq_ciscond_make_plan(int n, int p1, int q, int ncu, const int32_t *s_lo, const int32_t *s_hi, const int32_t *cond_ptr,
                                       const int32_t *cond_idx, const char *who, aq_ciscond_plan *pl, aq_cis_work *work, std::string *err) {
  aq_cis_work local;
  aq_cis_work &wk = work ? *work : local;
  aq_cis_plan cis{};
  const int rc = aq_cis_make_plan(n, p1, q, 0, ncu, s_lo, s_hi, 0, 0, 0, who, &cis, &wk, err);
  if (rc != AQ_OK) return rc;
  const int rcl = aq_ciscond_check_lists(cond_ptr, cond_idx, q, p1, AQ_ERR_UNSUPPORTED, who, err);
  if (rcl != AQ_OK) return rcl;
  int max_k = 0;
  for (int j = 0; j < wk.q_active; j++) {
    const int t = wk.order[(size_t)j];
    max_k = std::max(max_k, (int)(cond_ptr[t + 1] - cond_ptr[t]));
  }
  const int kc = aq_ciscond_kc(max_k);
  const long long panel = 8ll * (wk.q_active > 0 ? wk.q_active : 1) * n;
  if ((1ll + kc) * panel > AQ_CISCOND_PANEL_MAX) {
    if (err)
      *err = std::string(who) + ": the residual traits and the " + std::to_string(kc) + " basis panels (" +
             std::to_string((1ll + kc) * panel) + " bytes) exceed 4 GiB";
    return AQ_ERR_UNSUPPORTED;
  }
  pl->cis = cis;
  pl->kc = kc;
  pl->max_k = max_k;
  pl->lds_bytes = aq_ciscond_lds_bytes(kc);
  pl->streams = 1 + kc;
  pl->qo_bytes = kc * panel;
  pl->yo_bytes = panel;
  return AQ_OK;
}
