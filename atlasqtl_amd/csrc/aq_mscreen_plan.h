// aq_mscreen_plan.h -- the launch plan of the marginal screen r = cor(Xs[:, s], Yc[:, t]) over every predictor x trait pair
// (aq_prep_marginal, kernels in aq_mscreen_kernels.h): tile edge, tile counts, LDS and scratch size from n, p1, q, whether Yc
// has missing values and the device's CU count.  A pure function in the manner of aq_grm_plan.h: integer arithmetic only,
// no HIP call, no getenv.  aq_prep_marginal runs it before it allocates anything; aq_mscreen_plan_query exposes it on the
// C ABI without a device.
//
// Workgroup b of the plain grid n_tiles = tiles_p tiles_q owns the tile (tp, tq) = (b mod tiles_p, b / tiles_p): predictors
// [tile tp, tile tp + tile) against traits [tile tq, tile tq + tile), contracted over all n samples AQ_MSCREEN_NC at a time.
// Neighbouring workgroups share their panel of traits.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/atlasqtl_hip.h"

#define AQ_MSCREEN_NC 16            // samples staged in LDS per step
#define AQ_MSCREEN_STR 18           // doubles per LDS row: AQ_MSCREEN_NC + 2 (aq_screen_tile.h has the bank argument)
#define AQ_MSCREEN_TILE_MASKED 64   // three accumulator sets: 96 of the 512 registers of a lane; 128 x 128 would need 384

#if defined(__HIPCC__)
#define AQ_MSCREEN_HD __host__ __device__
#else
#define AQ_MSCREEN_HD
#endif

// static LDS of a workgroup: the panels of X and Y (and of the mask), rows of AQ_MSCREEN_STR doubles; the two columns of
// per-trait candidates (double r, int snp) that the four waves reduce through; the tile's Syy_t, cutoff and m_t
AQ_MSCREEN_HD constexpr int aq_mscreen_lds_bytes(int tile, bool masked) {
  return (masked ? 3 : 2) * tile * AQ_MSCREEN_STR * 8 + 2 * tile * (8 + 4) + tile * (8 + 8 + 4);
}

// force_tile > 0: that tile edge for complete Y (AQ_MSCREEN_TILE, tests), whatever the shape and the CU count say
static inline int aq_mscreen_make_plan(int n, int p1, int q, int masked, int ncu, int force_tile, const char *who, aq_mscreen_plan *pl,
                                       std::string *err) {
  if (n < 1 || p1 < 1 || q < 1 || ncu < 1 || (masked != 0 && masked != 1)) {
    if (err) *err = std::string(who) + ": n >= 1, p1 >= 1, q >= 1, ncu >= 1 and masked in {0, 1} required";
    return AQ_ERR_ARG;
  }
  if (force_tile != 0 && force_tile != 64 && force_tile != 128) {
    if (err) *err = std::string(who) + ": AQ_MSCREEN_TILE must be 64 or 128";
    return AQ_ERR_ARG;
  }
  int T;
  if (masked) {
    T = AQ_MSCREEN_TILE_MASKED;
  } else if (force_tile > 0) {
    T = force_tile;
  } else {
    // 128 x 128 tiles read each staged double 4 times per wave and halve the traffic of 64 x 64 tiles; they are worth it
    // once they alone give every CU a workgroup
    const long long big = (((long long)p1 + 127) / 128) * (((long long)q + 127) / 128);
    T = big >= (long long)ncu ? 128 : 64;
  }
  const long long tp = ((long long)p1 + T - 1) / T, tq = ((long long)q + T - 1) / T;
  if (tp * tq >= (1ll << 31)) {
    if (err) *err = std::string(who) + ": " + std::to_string(tp * tq) + " tiles exceed the grid";
    return AQ_ERR_UNSUPPORTED;
  }
  pl->tile = T;
  pl->sample_chunk = AQ_MSCREEN_NC;
  pl->tiles_p = (int32_t)tp;
  pl->tiles_q = (int32_t)tq;
  pl->masked = masked;
  pl->lds_bytes = aq_mscreen_lds_bytes(T, masked != 0);
  pl->n_tiles = tp * tq;
  pl->scratch_bytes = tp * (long long)q * (8 + 4);   // per row of tiles and trait: its best r (double) and predictor (int32)
  return AQ_OK;
}
