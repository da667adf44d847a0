// aq_predict_plan.h -- the launch plan of Yhat = Xt B, the fitted model applied to n_new rows of genotypes (aq_vb_predict,
// aq_vb_fitted, aq_predict; kernels in aq_predict_kernels.h): sample tiles and trait tiles per workgroup, predictor splits and
// the bytes of the operand panels and of the partial tiles, from n_new, p, q and the device's CU count.  A pure function in
// the manner of aq_grm_plan.h: integer arithmetic only, no HIP call, no getenv.  The entries run it before they allocate
// anything; aq_predict_plan_query exposes it on the C ABI without a device.
//
// Workgroup (b, g, s) of the grid (sample_blocks, trait_groups, splits) owns the sample tiles [b sample_tiles,
// (b + 1) sample_tiles), a quarter of them per wave, the trait tiles [g trait_tiles, (g + 1) trait_tiles) and the predictors
// of split s, chunks_per_split chunks of AQ_PREDICT_KC each, and writes its partial tiles to scratch
// [splits][ceil(q / 16)][n_pad][16].  A second kernel adds the partials of an entry in the order s = 0, 1, ...
#pragma once
#include <cstdint>
#include <string>

#include "../../include/atlasqtl_hip.h"
#include "aq_plan_const.h"     // AQ_N_MAX

#define AQ_PREDICT_KC 16           // predictors per step: one 16 x 16 block of B, 2 KB contiguous in gam and in mu
#define AQ_PREDICT_MAX_SPLITS 64
#define AQ_PREDICT_MIN_CHUNKS 8    // a split the plan chooses itself holds at least this many chunks
#define AQ_PREDICT_MAX_TILES 65535    // trait tiles (reduce kernel) and trait groups are the y dimension of a grid

static inline long long aq_predict_p_pad(int p) { return 16ll * (((long long)p + 15) / 16); }

// force_splits > 0: that many splits (AQ_PREDICT_SPLITS, tests), whatever p and the CU count say
static inline int aq_predict_make_plan(int n_new, int p, int q, int ncu, int force_splits, const char *who, aq_predict_plan *pl,
                                       std::string *err) {
  if (n_new < 1 || n_new > AQ_N_MAX || p < 1 || q < 1 || ncu < 1) {
    if (err)
      *err = std::string(who) + ": 1 <= n_new <= " + std::to_string(AQ_N_MAX) + " (AQ_N_MAX), p >= 1, q >= 1 and ncu >= 1 required";
    return AQ_ERR_ARG;
  }
  if (force_splits < 0 || force_splits > AQ_PREDICT_MAX_SPLITS) {
    if (err) *err = std::string(who) + ": AQ_PREDICT_SPLITS must lie in [1, " + std::to_string(AQ_PREDICT_MAX_SPLITS) + "]";
    return AQ_ERR_ARG;
  }
  const long long dbl = (long long)sizeof(double);
  const long long tiles_n = ((long long)n_new + 15) / 16, tiles_q = ((long long)q + 15) / 16;
  // accumulator rows per wave: a loaded block of B is used once per row, so as many as the samples fill (at most 4:
  // 4 x 2 accumulators and two sets of operands stay far below the register file)
  const long long ns = tiles_n > 8 ? 4 : tiles_n > 4 ? 2 : 1;
  const long long st = 4 * ns;
  const long long blocks = (tiles_n + st - 1) / st;
  // two trait tiles per workgroup halve the reads of Xt; one where that would leave CUs without a workgroup
  const long long tt = (tiles_q >= 2 && blocks * tiles_q >= 4ll * ncu) ? 2 : 1;
  const long long groups = (tiles_q + tt - 1) / tt;
  if (tiles_q > AQ_PREDICT_MAX_TILES) {
    if (err)
      *err = std::string(who) + ": q = " + std::to_string(q) + " exceeds " + std::to_string(16 * AQ_PREDICT_MAX_TILES) +
             " traits per call (the trait tiles are the y dimension of the grids)";
    return AQ_ERR_UNSUPPORTED;
  }
  const long long wgs = blocks * groups;
  const long long chunks = ((long long)p + AQ_PREDICT_KC - 1) / AQ_PREDICT_KC;
  long long S;
  if (force_splits > 0) {
    S = force_splits;
  } else {
    // two workgroups per CU keep the matrix pipe fed while one of them waits for its operands; the tiles alone may give that
    S = wgs >= 2ll * ncu ? 1 : (2ll * ncu + wgs - 1) / wgs;
    if (S > chunks / AQ_PREDICT_MIN_CHUNKS) S = chunks / AQ_PREDICT_MIN_CHUNKS;
    if (S > AQ_PREDICT_MAX_SPLITS) S = AQ_PREDICT_MAX_SPLITS;
    if (S < 1) S = 1;
  }
  const long long n_pad = 16 * st * blocks;
  pl->sample_tiles = (int32_t)st;
  pl->trait_tiles = (int32_t)tt;
  pl->sample_blocks = (int32_t)blocks;
  pl->trait_groups = (int32_t)groups;
  pl->splits = (int32_t)S;
  pl->chunk = AQ_PREDICT_KC;
  pl->chunks_per_split = (int32_t)((chunks + S - 1) / S);
  pl->n_pad = (int32_t)n_pad;
  pl->panel_bytes = n_pad * aq_predict_p_pad(p) * dbl;
  pl->scratch_bytes = S * tiles_q * n_pad * 16 * dbl;
  return AQ_OK;
}
