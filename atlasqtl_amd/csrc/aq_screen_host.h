// aq_screen_host.h -- the host side that the entries of the screen family share (aq_prep_marginal.hip,
// aq_prep_marginal_perm.hip and, beneath aq_cis_host.h, aq_prep_cis.hip, aq_prep_cis_cond.hip and aq_prep_cis_int.hip): the reader of the
// environment hooks, the per-trait sums with the decision whether any value is missing, the cutoff and the permutation rows of
// the timing hooks, the check of r2_cut, the copy-back of the capped pair table, and the step from the runtime parity of n to
// the kernels' A16 template argument.  Static functions: each unit has its own copy.  The including unit includes its kernel
// header, and with it aq_screen_tile.h, as well.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <vector>
#include "aq_prep.h"          // aq_prep, aq_time_launches; aq_internal.h: aq_fail, AQ_HIP, aq_need_device, aq_need_acc_layout, AqDev
#include "aq_screen_tile.h"   // aq_k_ms_traitstats

// an environment variable that forces a plan field: 0 when it is not set, -1 when it is no number >= 1 (the planner's message)
static int aq_screen_env(const char *name) {
  const char *e = getenv(name);
  if (!e) return 0;
  const int v = atoi(e);
  return v < 1 ? -1 : v;
}

// Syy_t and m_t of the handle's traits on the device (allocated here) and m_t on the host; whether any value of Yc is missing,
// over ALL traits, so that every entry picks the same instance and computes the same bits; the CU count the planners take
static int aq_screen_trait_stats(aq_prep *h, AqDev<double> *syy, AqDev<int> *mt, std::vector<int> *mt_host, int *masked, int *ncu) {
  const size_t q = (size_t)h->q;
  AQ_TRY(syy->alloc(q));
  AQ_TRY(mt->alloc(q));
  hipLaunchKernelGGL(aq_k_ms_traitstats, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, 0, h->Yc.get(), h->n, h->q, syy->get(), mt->get());
  AQ_HIP(hipGetLastError());
  mt_host->resize(q);
  AQ_HIP(hipMemcpy(mt_host->data(), mt->get(), q * sizeof(int), hipMemcpyDeviceToHost));
  *masked = 0;
  for (size_t t = 0; t < q; t++) *masked |= (*mt_host)[t] < h->n;
  AQ_HIP(hipDeviceGetAttribute(ncu, hipDeviceAttributeMultiprocessorCount, h->device));
  if (*ncu <= 0) *ncu = 256;
  return AQ_OK;
}

// the cutoff of the timing hooks: t^2 = 40 (p about 1e-9 at large df), r2_cut = 40 / (40 + df), +inf where df < 1
static double aq_screen_time_cut(int df) {
  return df >= 1 ? 40.0 / (40.0 + (double)df) : std::numeric_limits<double>::infinity();
}

// the rows of the timing hooks: `rows` pseudo-random permutations of 0 ... n - 1, a Fisher-Yates shuffle driven by a 64-bit LCG
static std::vector<int32_t> aq_screen_time_perms(size_t rows, size_t n) {
  std::vector<int32_t> perm(rows * n);
  uint64_t state = 0x9e3779b97f4a7c15ull;
  for (size_t r = 0; r < rows; r++) {
    int32_t *row = perm.data() + r * n;
    for (size_t i = 0; i < n; i++) row[i] = (int32_t)i;
    for (size_t i = n; i > 1; i--) {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      const size_t j = (size_t)((state >> 33) % i);
      const int32_t tmp = row[i - 1];
      row[i - 1] = row[j];
      row[j] = tmp;
    }
  }
  return perm;
}

static int aq_screen_need_cut(const double *r2_cut, int q, const char *who) {
  for (int t = 0; t < q; t++)
    if (std::isnan(r2_cut[t])) return aq_fail(AQ_ERR_ARG, std::string(who) + ": r2_cut[" + std::to_string(t) + "] is NaN");
  return AQ_OK;
}

// the rows of the pair table that exist, min(count, cap), into those of snp, trait and r that are given
static int aq_screen_copy_pairs(unsigned long long count, int64_t cap, const AqDev<int32_t> &dsnp, const AqDev<int32_t> &dtrait,
                                const AqDev<double> &dr, int32_t *snp, int32_t *trait, double *r) {
  const size_t rows = count < (unsigned long long)cap ? (size_t)count : (size_t)cap;
  if (rows > 0) {
    if (snp) AQ_HIP(hipMemcpy(snp, dsnp.get(), rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (trait) AQ_HIP(hipMemcpy(trait, dtrait.get(), rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (r) AQ_HIP(hipMemcpy(r, dr.get(), rows * sizeof(double), hipMemcpyDeviceToHost));
  }
  return AQ_OK;
}

// f(std::true_type) for even n, where every column starts at a multiple of 16 bytes (the kernels' A16), else f(std::false_type):
//   aq_screen_a16(n, [&](auto a16) { hipLaunchKernelGGL((kernel<..., decltype(a16)::value>), ...); });
template <typename F>
static void aq_screen_a16(int n, F f) {
  if ((n & 1) == 0)
    f(std::true_type{});
  else
    f(std::false_type{});
}
