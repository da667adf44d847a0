// aq_cis_plan.h -- the launch plan of the cis scan (aq_prep_cis, aq_prep_cis_perm; kernels in aq_cis_kernels.h): every trait is
// tested only against the predictors of its own window s_lo[t] <= s < s_hi[t], a band of the p1 x q matrix.  From n, p1, q,
// whether Yc has missing values, the device's CU count, the windows and the number of permutations: the order of the traits,
// the trait tiles, the list of work items that takes the place of the plain grid of aq_mscreen_plan.h, LDS and scratch sizes
// and, for permutations, PB, the batch and the launches by the rules of aq_msperm_plan.h.  A pure function in the manner of
// aq_mscreen_plan.h: integer arithmetic only, no HIP call, no getenv.  aq_prep_cis runs it before it allocates anything;
// aq_cis_plan_query exposes it on the C ABI without a device.  The check of the windows is here too: it is host arithmetic.
//
// order: a permutation of the traits.  Those with a non-empty window come first, sorted by (s_lo, s_hi, t); those with an
// empty window come last, by t, and belong to no tile.  Trait tile k holds the traits order[64 k] ... order[64 k + 63] (fewer
// in the last tile) and has the union range [L_k, H_k) of their windows.  Its work items are (k, p0), p0 = L_k, L_k + 64, ...
// < H_k: predictors [p0, p0 + 64) against the tile's traits.  The items of tile k are first_item[k] ... first_item[k + 1] - 1
// of the two int32 arrays item_tile and item_p0, ascending in p0; W items in all, W < 2^31.  Every in-window pair lies in
// exactly one item: p0 + 64 steps cover [L_k, H_k) without overlap, and the window of a tile's trait lies inside it.
// One tile edge, 64: windows are narrow, and a 128 tile would stage mostly pairs outside them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "aq_mscreen_plan.h"

#define AQ_CIS_TILE 64
#define AQ_CIS_YP_MAX (1ll << 30)          // bytes of the gathered panels of a launch, and of its scratch
#define AQ_CIS_PB_MAX 4
#define AQ_CIS_PB_MASKED_MAX 2             // three accumulator sets per permutation: 96 registers each

// static LDS of a workgroup of the scan: the panels of X and Y (and of the mask), rows of AQ_MSCREEN_STR doubles; the two
// columns of per-trait candidates (double r, int snp); per trait Syy_t, the cutoff, m_t, s_lo, s_hi and the trait's own index
AQ_MSCREEN_HD constexpr int aq_cis_lds_bytes(bool masked) {
  return (masked ? 3 : 2) * AQ_CIS_TILE * AQ_MSCREEN_STR * 8 + 2 * AQ_CIS_TILE * (8 + 4) + AQ_CIS_TILE * (8 + 8 + 4 + 4 + 4 + 4);
}

// ... of the permutation kernel: the panel of X, PB panels of Y (and of the mask); per trait Syy_t, m_t, s_lo, s_hi and its
// index; the two columns of per-(permutation, trait) maxima
AQ_MSCREEN_HD constexpr int aq_cis_perm_lds_bytes(bool masked, int pb) {
  return (1 + (masked ? 2 : 1) * pb) * AQ_CIS_TILE * AQ_MSCREEN_STR * 8 + AQ_CIS_TILE * (8 + 4 + 4 + 4 + 4) + 2 * pb * AQ_CIS_TILE * 8;
}

AQ_MSCREEN_HD constexpr bool aq_cis_instance(bool masked, int pb) {
  return masked ? (pb == 1 || pb == 2) : (pb == 1 || pb == 2 || pb == 4);
}

// scratch of one permutation of a launch: the key of max r^2 and max r^2 itself per trait, and its row of perm
static inline long long aq_cis_scratch_per_perm(int n, int q) { return 16ll * q + 4ll * n; }

// what the plan struct does not hold: the order and the work list
struct aq_cis_work {
  int q_active = 0;                        // traits with a non-empty window: order[0 ... q_active - 1]
  std::vector<int32_t> order;              // q
  std::vector<int32_t> tile_lo, tile_hi;   // per trait tile: L_k, H_k
  std::vector<int32_t> first_item;         // trait tiles + 1
  std::vector<int32_t> item_tile, item_p0; // W each
};

// 0 <= s_lo[t] <= s_hi[t] <= p1 for every trait; else the trait at fault
static inline int aq_cis_check_windows(const int32_t *s_lo, const int32_t *s_hi, int q, int p1, const char *who, std::string *err) {
  for (int t = 0; t < q; t++) {
    const long long lo = s_lo[t], hi = s_hi[t];
    if (lo < 0 || hi < 0 || lo > p1 || hi > p1) {
      if (err)
        *err = std::string(who) + ": the window of trait " + std::to_string(t) + ", [" + std::to_string(lo) + ", " + std::to_string(hi) +
               "), is outside [0, " + std::to_string(p1) + "]";
      return AQ_ERR_ARG;
    }
    if (lo > hi) {
      if (err)
        *err = std::string(who) + ": s_lo > s_hi for trait " + std::to_string(t) + " (" + std::to_string(lo) + " > " + std::to_string(hi) + ")";
      return AQ_ERR_ARG;
    }
  }
  return AQ_OK;
}

// n_perm = 0: the scan alone.  force_pb, force_batch > 0: AQ_CIS_PB, AQ_CIS_BATCH (tests); < 0: set, but not a number; both
// are looked at only when n_perm > 0.  work may be NULL (the query).
static inline int aq_cis_make_plan(int n, int p1, int q, int masked, int ncu, const int32_t *s_lo, const int32_t *s_hi, int n_perm,
                                   int force_pb, int force_batch, const char *who, aq_cis_plan *pl, aq_cis_work *work, std::string *err) {
  const std::string w(who);
  if (n < 1 || p1 < 1 || q < 1 || ncu < 1 || (masked != 0 && masked != 1)) {
    if (err) *err = w + ": n >= 1, p1 >= 1, q >= 1, ncu >= 1 and masked in {0, 1} required";
    return AQ_ERR_ARG;
  }
  if (!s_lo || !s_hi) {
    if (err) *err = w + ": NULL s_lo or s_hi";
    return AQ_ERR_ARG;
  }
  if (n_perm < 0) {
    if (err) *err = w + ": n_perm >= 0 required, " + std::to_string(n_perm) + " given";
    return AQ_ERR_ARG;
  }
  const int rcw = aq_cis_check_windows(s_lo, s_hi, q, p1, who, err);
  if (rcw != AQ_OK) return rcw;
  constexpr int T = AQ_CIS_TILE;
  aq_cis_work local;
  aq_cis_work &wk = work ? *work : local;
  wk = aq_cis_work{};
  wk.order.reserve((size_t)q);
  long long pairs = 0;
  for (int t = 0; t < q; t++)
    if (s_hi[t] > s_lo[t]) {
      wk.order.push_back(t);
      pairs += (long long)s_hi[t] - (long long)s_lo[t];
    }
  std::sort(wk.order.begin(), wk.order.end(), [&](int32_t a, int32_t b) {
    if (s_lo[a] != s_lo[b]) return s_lo[a] < s_lo[b];
    if (s_hi[a] != s_hi[b]) return s_hi[a] < s_hi[b];
    return a < b;
  });
  const int qa = (int)wk.order.size();
  wk.q_active = qa;
  for (int t = 0; t < q; t++)
    if (s_hi[t] == s_lo[t]) wk.order.push_back(t);
  const int tiles = (qa + T - 1) / T;
  wk.tile_lo.resize((size_t)tiles);
  wk.tile_hi.resize((size_t)tiles);
  wk.first_item.resize((size_t)tiles + 1);
  long long W = 0;
  for (int k = 0; k < tiles; k++) {
    int lo = s_lo[wk.order[(size_t)T * k]], hi = 0;          // sorted by s_lo: the first trait has the smallest
    for (int j = T * k; j < T * k + T && j < qa; j++) hi = std::max(hi, (int)s_hi[wk.order[(size_t)j]]);
    wk.tile_lo[(size_t)k] = lo;
    wk.tile_hi[(size_t)k] = hi;
    W += ((long long)hi - lo + T - 1) / T;
  }
  if (W >= (1ll << 31)) {
    if (err) *err = w + ": " + std::to_string(W) + " work items exceed the grid";
    return AQ_ERR_UNSUPPORTED;
  }
  wk.item_tile.reserve((size_t)W);
  wk.item_p0.reserve((size_t)W);
  for (int k = 0; k < tiles; k++) {
    wk.first_item[(size_t)k] = (int32_t)wk.item_tile.size();
    for (long long p0 = wk.tile_lo[(size_t)k]; p0 < wk.tile_hi[(size_t)k]; p0 += T) {
      wk.item_tile.push_back(k);
      wk.item_p0.push_back((int32_t)p0);
    }
  }
  wk.first_item[(size_t)tiles] = (int32_t)W;

  int pb = 0;
  long long batch = 0, launches = 0, panel = 0, per = 0;
  if (n_perm > 0) {
    if (force_pb != 0 && !aq_cis_instance(masked != 0, force_pb)) {
      if (err) *err = w + ": AQ_CIS_PB must be 1, 2 or 4 for complete Y, and 1 or 2 for Y with missing values";
      return AQ_ERR_ARG;
    }
    panel = 8ll * (qa > 0 ? qa : 1) * n;                     // the traits without a window are not gathered
    per = aq_cis_scratch_per_perm(n, q);
    if (panel > AQ_CIS_YP_MAX || per > AQ_CIS_YP_MAX) {
      if (err) *err = w + ": one permuted panel of Y (" + std::to_string(panel) + " bytes) exceeds 1 GiB";
      return AQ_ERR_UNSUPPORTED;
    }
    long long most = AQ_CIS_YP_MAX / panel;
    if (AQ_CIS_YP_MAX / per < most) most = AQ_CIS_YP_MAX / per;
    // PB as measured on an MI355X at n = 1000, p1 = 50 000, q = 10 000 with windows of about 470 and 2270 predictors (DESIGN.md
    // section 9): complete Y is fastest with PB = 2 (0.33 / 0.88 ms a permutation; 0.36 / 0.94 with PB = 1, 0.33 / 0.94 with
    // PB = 4); masked Y with PB = 1 (0.78 / 2.42 ms; 0.81 / 2.52 with PB = 2): the defaults of aq_msperm_plan.h at tile 64
    pb = force_pb > 0 ? force_pb : masked ? 1 : 2;
    if (most < pb) {
      if (force_pb > 0) {
        if (err) *err = w + ": AQ_CIS_PB = " + std::to_string(pb) + " panels of Y exceed 1 GiB";
        return AQ_ERR_ARG;
      }
      pb = 1;
    }
    const long long grid_most = (((1ll << 31) - 1) / (W > 0 ? W : 1)) * pb;   // groups W < 2^31
    if (grid_most < most) most = grid_most;
    const long long need = (((long long)n_perm + pb - 1) / pb) * pb;          // no more than the permutations asked for
    if (need < most) most = need;
    batch = (most / pb) * pb;
    if (batch < pb) {
      if (err) *err = w + ": " + std::to_string(W) + " work items exceed the grid";
      return AQ_ERR_UNSUPPORTED;
    }
    if (force_batch != 0) {
      if (force_batch < 0 || force_batch % pb != 0 || (long long)force_batch > (most / pb) * pb) {
        if (err)
          *err = w + ": AQ_CIS_BATCH must be a multiple of PB = " + std::to_string(pb) + " between " + std::to_string(pb) + " and " +
                 std::to_string((most / pb) * pb);
        return AQ_ERR_ARG;
      }
      batch = force_batch;
    }
    launches = ((long long)n_perm + batch - 1) / batch;
  }
  pl->tile = T;
  pl->sample_chunk = AQ_MSCREEN_NC;
  pl->trait_tiles = tiles;
  pl->q_active = qa;
  pl->masked = masked;
  pl->lds_bytes = aq_cis_lds_bytes(masked != 0);
  pl->perm_lds_bytes = pb > 0 ? aq_cis_perm_lds_bytes(masked != 0, pb) : 0;
  pl->pb = pb;
  pl->batch = (int32_t)batch;
  pl->launches = (int32_t)launches;
  pl->n_items = W;
  pl->window_pairs = pairs;
  pl->staged_pairs = (long long)T * T * W;
  pl->yp_bytes = batch * panel;
  pl->scratch_bytes = W * (long long)T * (8 + 4) + batch * per;   // each item's best predictor per trait; the permutations' rows
  return AQ_OK;
}
