// aq_msperm_plan.h -- the launch plan of the permutation nulls of the marginal screen (aq_prep_marginal_perm, kernels in
// aq_msperm_kernels.h): tile edge, permutations per workgroup (PB), permutations per launch (batch), launches, tile counts,
// LDS, the bytes of the gathered panels Yp and of the scratch, from n, p1, q, whether Yc has missing values, the device's CU
// count and the number of permutations.  A pure function in the manner of aq_mscreen_plan.h: integer arithmetic only, no HIP
// call, no getenv.  aq_prep_marginal_perm runs it before it allocates anything; aq_msperm_plan_query exposes it on the C ABI
// without a device.  The check of the permutation rows is here too, for the same reason: it is host arithmetic.
//
// A launch covers `batch` permutations, gathered as Yp[batch][q][n].  Workgroup w of the plain grid n_tiles groups,
// groups = ceil(permutations of the launch / PB), owns the tile (tp, tq) of aq_mscreen_plan.h, (tp, tq) = (v mod tiles_p,
// v / tiles_p) with v = w mod n_tiles, and the PB permutations PB g ... PB g + PB - 1 of group g = w / n_tiles; those at or
// beyond the launch's count are not computed.
//
// The instances (aq_msperm_kernels.h has the register argument): complete Y at tile 64 with PB 1, 2, 4 and at tile 128 with
// PB 1; masked Y at tile 64 with PB 1, 2.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "aq_mscreen_plan.h"

#define AQ_MSPERM_YP_MAX (1ll << 30)       // bytes of Yp, and of the per-launch scratch
#define AQ_MSPERM_PB_MAX 4
#define AQ_MSPERM_PB_MASKED_MAX 2          // three accumulator sets per permutation: 96 registers each

// static LDS of a workgroup: the panel of X, PB panels of Y (and of the mask), rows of AQ_MSCREEN_STR doubles; the tile's
// Syy_t, cutoff and m_t; the two columns of per-(permutation, trait) maxima that the waves of a tile row reduce through
AQ_MSCREEN_HD constexpr int aq_msperm_lds_bytes(int tile, bool masked, int pb) {
  return (1 + (masked ? 2 : 1) * pb) * tile * AQ_MSCREEN_STR * 8 + tile * (8 + 8 + 4) + 2 * pb * tile * 8;
}

AQ_MSCREEN_HD constexpr bool aq_msperm_instance(int tile, bool masked, int pb) {
  return masked ? (tile == AQ_MSCREEN_TILE_MASKED && (pb == 1 || pb == 2)) : tile == 128 ? pb == 1 : (tile == 64 && (pb == 1 || pb == 2 || pb == 4));
}

// scratch of one permutation of a launch: count[p1] (uint32), the key of max r^2 and max r^2 itself per trait, n_undef,
// hs_max, n_sel, and its row of perm
static inline long long aq_msperm_scratch_per_perm(int n, int p1, int q) {
  return 4ll * p1 + 16ll * q + 24 + 4ll * n;
}

// force_tile, force_pb, force_batch > 0: AQ_MSCREEN_TILE, AQ_MSPERM_PB, AQ_MSPERM_BATCH (tests); < 0: set, but not a number
static inline int aq_msperm_make_plan(int n, int p1, int q, int masked, int ncu, int n_perm, int force_tile, int force_pb,
                                      int force_batch, const char *who, aq_msperm_plan *pl, std::string *err) {
  const std::string w(who);
  if (n_perm < 1) {
    if (err) *err = w + ": n_perm >= 1 required, " + std::to_string(n_perm) + " given";
    return AQ_ERR_ARG;
  }
  aq_mscreen_plan ms{};
  const int rc = aq_mscreen_make_plan(n, p1, q, masked, ncu, force_tile, who, &ms, err);
  if (rc != AQ_OK) return rc;
  const int T = ms.tile;
  if (force_pb != 0 && !aq_msperm_instance(T, masked != 0, force_pb)) {
    if (err)
      *err = w + ": AQ_MSPERM_PB must be 1, 2 or 4 for complete Y at tile 64, 1 at tile 128, and 1 or 2 for Y with missing values";
    return AQ_ERR_ARG;
  }
  const long long panel = 8ll * q * n, per = aq_msperm_scratch_per_perm(n, p1, q);
  if (panel > AQ_MSPERM_YP_MAX || per > AQ_MSPERM_YP_MAX) {
    if (err) *err = w + ": one permuted panel of Y (" + std::to_string(panel) + " bytes) exceeds 1 GiB";
    return AQ_ERR_UNSUPPORTED;
  }
  // the most permutations one launch may hold: Yp and the scratch within 1 GiB each, and the grid within 2^31 workgroups
  long long most = AQ_MSPERM_YP_MAX / panel;
  if (AQ_MSPERM_YP_MAX / per < most) most = AQ_MSPERM_YP_MAX / per;
  // PB as measured on an MI355X at n = 1000, p1 = 50 000, q = 10 000: complete Y at tile 64 is fastest
  // with PB = 2 (16.5 ms a permutation; 18.3 with PB = 1, 17.6 with PB = 4); masked Y with PB = 1 (46.0 ms; 47.7 with PB = 2,
  // whose 192 accumulator registers leave the compiler 64 for everything else); tile 128 has PB = 1 only
  int pb = force_pb > 0 ? force_pb : (!masked && T == 64) ? 2 : 1;
  if (most < pb) {
    if (force_pb > 0) {
      if (err) *err = w + ": AQ_MSPERM_PB = " + std::to_string(pb) + " panels of Y exceed 1 GiB";
      return AQ_ERR_ARG;
    }
    pb = 1;
  }
  const long long grid_most = (((1ll << 31) - 1) / ms.n_tiles) * pb;      // groups n_tiles < 2^31
  if (grid_most < most) most = grid_most;
  const long long need = (((long long)n_perm + pb - 1) / pb) * pb;        // no more than the permutations asked for
  if (need < most) most = need;
  long long batch = (most / pb) * pb;
  if (batch < pb) {
    if (err) *err = w + ": " + std::to_string(ms.n_tiles) + " tiles exceed the grid";
    return AQ_ERR_UNSUPPORTED;
  }
  if (force_batch != 0) {
    if (force_batch < 0 || force_batch % pb != 0 || (long long)force_batch > (most / pb) * pb) {
      if (err)
        *err = w + ": AQ_MSPERM_BATCH must be a multiple of PB = " + std::to_string(pb) + " between " + std::to_string(pb) + " and " +
               std::to_string((most / pb) * pb);
      return AQ_ERR_ARG;
    }
    batch = force_batch;
  }
  pl->tile = T;
  pl->pb = pb;
  pl->batch = (int32_t)batch;
  pl->launches = (int32_t)(((long long)n_perm + batch - 1) / batch);
  pl->tiles_p = ms.tiles_p;
  pl->tiles_q = ms.tiles_q;
  pl->masked = masked;
  pl->lds_bytes = aq_msperm_lds_bytes(T, masked != 0, pb);
  pl->yp_bytes = batch * panel;
  pl->scratch_bytes = batch * per;
  return AQ_OK;
}

// every row of perm ([n_perm][n]) is a permutation of 0 ... n - 1; else the row and the index at fault
static inline int aq_msperm_check_rows(const int32_t *perm, int n_perm, int n, const char *who, std::string *err) {
  std::vector<uint8_t> seen((size_t)n);
  for (int b = 0; b < n_perm; b++) {
    std::fill(seen.begin(), seen.end(), (uint8_t)0);
    const int32_t *row = perm + (size_t)b * (size_t)n;
    for (int i = 0; i < n; i++) {
      const int32_t v = row[i];
      if (v < 0 || v >= n || seen[(size_t)v]) {
        if (err)
          *err = std::string(who) + ": row " + std::to_string(b) + " of perm is not a permutation of 0 ... " + std::to_string(n - 1) +
                 ": index " + std::to_string(v) + " at position " + std::to_string(i) +
                 ((v < 0 || v >= n) ? " is out of range" : " is repeated");
        return AQ_ERR_ARG;
      }
      seen[(size_t)v] = 1;
    }
  }
  return AQ_OK;
}
