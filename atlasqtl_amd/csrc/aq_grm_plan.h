// aq_grm_plan.h -- the launch plan of the genetic relationship matrix K = Xs Xs' / p1 (aq_prep_grm, kernels in
// aq_grm_kernels.h): tile edge, number of predictor splits and scratch size from n, p1, the device's CU count and its free
// memory.  A pure function in the manner of aq_plan.h: integer arithmetic only, no HIP call, no getenv.  aq_prep_grm runs it
// before it allocates anything; aq_grm_plan_query exposes it on the C ABI without a device.
//
// One triangle of T x T output tiles is computed (tile row ti >= tile column tj); workgroup (t, s) of the grid
// (n_tiles, splits) owns tile t = ti (ti + 1) / 2 + tj and the predictors of split s, chunks_per_split chunks of AQ_GRM_KC
// each, and writes its partial tile to scratch.  A second kernel adds the partials of a tile in the order s = 0, 1, ...
#pragma once
#include <cstdint>
#include <string>

#include "../../include/atlasqtl_hip.h"

#define AQ_GRM_MAX_N 10240     // K is 0.84 GB there and its eigen-decomposition is on the host
#define AQ_GRM_KC 16           // predictors staged in LDS per step
#define AQ_GRM_MAX_SPLITS 64
#define AQ_GRM_MIN_CHUNKS 8    // a split the plan chooses itself holds at least this many chunks

#if defined(__HIPCC__)
#define AQ_GRM_HD __host__ __device__
#else
#define AQ_GRM_HD
#endif

// tile t of the triangle -> (ti, tj), ti >= tj: t = ti (ti + 1) / 2 + tj.  Exact for every t < 2^30.
AQ_GRM_HD static inline void aq_grm_tile_rc(int t, int *ti, int *tj) {
  int r = 0;
  for (int bit = 1 << 15; bit > 0; bit >>= 1) {   // the largest r with r (r + 1) / 2 <= t, bit by bit
    const long long c = (long long)(r + bit);
    if (c * (c + 1) / 2 <= (long long)t) r += bit;
  }
  *ti = r;
  *tj = t - (int)((long long)r * (r + 1) / 2);
}

// `who`: the entry that reports the error
static inline int aq_grm_check_n(int n, const char *who, std::string *err) {
  if (n > AQ_GRM_MAX_N) {
    if (err)
      *err = std::string(who) + ": n = " + std::to_string(n) + " exceeds " + std::to_string(AQ_GRM_MAX_N) +
             " samples: the n x n matrix and its eigen-decomposition on the host are not supported beyond that";
    return AQ_ERR_UNSUPPORTED;
  }
  return AQ_OK;
}

// force_splits > 0: that many splits (AQ_GRM_SPLITS, tests), whatever p1 and the CU count say
static inline int aq_grm_make_plan(int n, int p1, int ncu, long long free_bytes, int force_splits, const char *who, aq_grm_plan *pl,
                                   std::string *err) {
  if (n < 2 || p1 < 1 || ncu < 1 || free_bytes < 0) {
    if (err) *err = std::string(who) + ": n >= 2, p1 >= 1, ncu >= 1 and free_bytes >= 0 required";
    return AQ_ERR_ARG;
  }
  if (force_splits < 0 || force_splits > AQ_GRM_MAX_SPLITS) {
    if (err) *err = std::string(who) + ": AQ_GRM_SPLITS must lie in [1, " + std::to_string(AQ_GRM_MAX_SPLITS) + "]";
    return AQ_ERR_ARG;
  }
  const int rc = aq_grm_check_n(n, who, err);
  if (rc != AQ_OK) return rc;
  // 128 x 128 tiles read each staged double 8 times per wave pair and halve the traffic of 64 x 64 tiles; below n = 257
  // they would be mostly padding
  const int T = n > 256 ? 128 : 64;
  const int nt = (n + T - 1) / T;
  const long long n_tiles = (long long)nt * (nt + 1) / 2;
  const long long chunks = ((long long)p1 + AQ_GRM_KC - 1) / AQ_GRM_KC;
  const long long tile_bytes = (long long)T * T * (long long)sizeof(double);
  const long long k_bytes = (long long)n * n * (long long)sizeof(double);
  const long long room = (free_bytes - k_bytes) / (n_tiles * tile_bytes);   // splits whose scratch fits next to K
  long long S;
  if (force_splits > 0) {
    S = force_splits;
  } else {
    // two workgroups per CU keep the matrix pipe fed while one of them stages; tiles alone may give that
    S = n_tiles >= 2ll * ncu ? 1 : (2ll * ncu + n_tiles - 1) / n_tiles;
    if (S > chunks / AQ_GRM_MIN_CHUNKS) S = chunks / AQ_GRM_MIN_CHUNKS;
    if (S > AQ_GRM_MAX_SPLITS) S = AQ_GRM_MAX_SPLITS;
    if (S > room) S = room;
    if (S < 1) S = 1;
  }
  if (room < S) {
    if (err)
      *err = std::string(who) + ": K and the partial tiles need " + std::to_string(k_bytes + S * n_tiles * tile_bytes) +
             " bytes of device memory, " + std::to_string(free_bytes) + " are free";
    return AQ_ERR_DEVICE;
  }
  pl->tile = T;
  pl->tiles_per_edge = nt;
  pl->n_tiles = (int32_t)n_tiles;
  pl->splits = (int32_t)S;
  pl->chunk = AQ_GRM_KC;
  pl->chunks_per_split = (int32_t)((chunks + S - 1) / S);
  pl->scratch_bytes = S * n_tiles * tile_bytes;
  pl->k_bytes = k_bytes;
  return AQ_OK;
}
