// aq_pcs_plan.h -- the launch plan of one application of the relationship operator Z = Xs (Xs' Q) / p1 to a block of L vectors
// (aq_prep_grm_apply, kernels in aq_pcs_kernels.h): padded block width, predictor panels of the first product, sample tiles and
// predictor splits of the second, and the bytes of T, of the partial tiles and of the operands, from n, p1, L, the device's CU
// count and its free memory.  A pure function in the manner of aq_grm_plan.h: integer arithmetic only, no HIP call, no getenv.
// aq_prep_grm_apply runs it before it allocates anything; aq_pcs_plan_query exposes it on the C ABI without a device.
//
// First product, T = Xs' Q: workgroup b of a grid of n_panels owns the predictors [b panel, (b + 1) panel) and all lp columns
// and walks the n_pad samples sample_chunk at a time.  Second product, Z = Xs T / p1: workgroup (t, s) of the grid
// (n_tiles, splits) owns the samples [t tile, (t + 1) tile), all lp columns and the predictors of split s, chunks_per_split
// chunks of AQ_PCS_KC each, and writes its partial tile to scratch; a third kernel adds the partials in the order s = 0, 1, ...
// Unlike K itself, none of this grows as n^2: there is no limit on n here beyond the handle's own (AQ_N_MAX).
#pragma once
#include <cstdint>
#include <string>

#include "../../include/atlasqtl_hip.h"

#define AQ_PCS_MAX_L 128       // vectors per block: k <= 96 components and their oversampling
#define AQ_PCS_PJ 64           // predictors per workgroup of the first product (16 per wave)
#define AQ_PCS_NC 32           // samples of Q staged in LDS per step of the first product
#define AQ_PCS_TS 64           // samples per workgroup of the second product (16 per wave)
#define AQ_PCS_KC 16           // predictors staged in LDS per step of the second product
#define AQ_PCS_MAX_SPLITS 64
#define AQ_PCS_MIN_CHUNKS 8    // a split the plan chooses itself holds at least this many chunks

// force_splits > 0: that many splits (AQ_PCS_SPLITS, tests), whatever p1 and the CU count say
static inline int aq_pcs_make_plan(int n, int p1, int L, int ncu, long long free_bytes, int force_splits, const char *who, aq_pcs_plan *pl,
                                   std::string *err) {
  if (L < 1 || L > AQ_PCS_MAX_L) {
    if (err) *err = std::string(who) + ": L must lie in [1, " + std::to_string(AQ_PCS_MAX_L) + "], " + std::to_string(L) + " given";
    return AQ_ERR_ARG;
  }
  if (n < 2 || p1 < 1 || ncu < 1 || free_bytes < 0) {
    if (err) *err = std::string(who) + ": n >= 2, p1 >= 1, ncu >= 1 and free_bytes >= 0 required";
    return AQ_ERR_ARG;
  }
  if (force_splits < 0 || force_splits > AQ_PCS_MAX_SPLITS) {
    if (err) *err = std::string(who) + ": AQ_PCS_SPLITS must lie in [1, " + std::to_string(AQ_PCS_MAX_SPLITS) + "]";
    return AQ_ERR_ARG;
  }
  const long long dbl = (long long)sizeof(double);
  const long long lp = 16ll * ((L + 15) / 16);
  const long long n_panels = ((long long)p1 + AQ_PCS_PJ - 1) / AQ_PCS_PJ;
  const long long n_pad = AQ_PCS_NC * (((long long)n + AQ_PCS_NC - 1) / AQ_PCS_NC);
  const long long n_tiles = ((long long)n + AQ_PCS_TS - 1) / AQ_PCS_TS;
  const long long chunks = ((long long)p1 + AQ_PCS_KC - 1) / AQ_PCS_KC;
  const long long t_bytes = n_panels * AQ_PCS_PJ * lp * dbl;            // every panel whole: rows >= p1 are written as 0.0
  const long long io_bytes = (2ll * n * L + n_pad * lp) * dbl;          // Q and Z as given, Q row-major and padded
  const long long tile_bytes = (long long)AQ_PCS_TS * lp * dbl;
  const long long room = (free_bytes - t_bytes - io_bytes) / (n_tiles * tile_bytes);   // splits whose scratch fits next to them
  long long S;
  if (force_splits > 0) {
    S = force_splits;
  } else {
    // two workgroups per CU keep the matrix pipe fed while one of them stages; the sample tiles alone may give that
    S = n_tiles >= 2ll * ncu ? 1 : (2ll * ncu + n_tiles - 1) / n_tiles;
    if (S > chunks / AQ_PCS_MIN_CHUNKS) S = chunks / AQ_PCS_MIN_CHUNKS;
    if (S > AQ_PCS_MAX_SPLITS) S = AQ_PCS_MAX_SPLITS;
    if (S > room) S = room;
    if (S < 1) S = 1;
  }
  if (room < S) {
    if (err)
      *err = std::string(who) + ": T, the operands and the partial tiles need " + std::to_string(t_bytes + io_bytes + S * n_tiles * tile_bytes) +
             " bytes of device memory, " + std::to_string(free_bytes) + " are free";
    return AQ_ERR_DEVICE;
  }
  pl->lp = (int32_t)lp;
  pl->panel = AQ_PCS_PJ;
  pl->n_panels = (int32_t)n_panels;
  pl->sample_chunk = AQ_PCS_NC;
  pl->n_pad = (int32_t)n_pad;
  pl->tile = AQ_PCS_TS;
  pl->n_tiles = (int32_t)n_tiles;
  pl->splits = (int32_t)S;
  pl->chunk = AQ_PCS_KC;
  pl->chunks_per_split = (int32_t)((chunks + S - 1) / S);
  pl->t_bytes = t_bytes;
  pl->scratch_bytes = S * n_tiles * tile_bytes;
  pl->io_bytes = io_bytes;
  return AQ_OK;
}
