// aq_finemap_plan.h -- the launch plan of the cis fine-mapping (aq_prep_cis_finemap; kernels in aq_finemap_kernels.h): the
// order of the traits, the trait tiles and the work items are those of aq_cis_plan.h, complete Y, no permutations.  On top of
// them: the number L of single effects, and how many consecutive trait tiles run in lockstep as one batch.  A pure function in
// the manner of aq_cis_plan.h: integer arithmetic only, no HIP call, no getenv (the entry reads AQ_FM_BATCH_TILES and hands
// the value in).
//
// What a batch holds on the device.  Per work item w of its tiles a 64 x 64 block of each of alpha and mu per effect, the
// state, 2 L 64 64 8 bytes; one 64 x 64 block of x's, the band buffer Z; per trait the residual panel R, the running residual
// Rf and the L fits, (L + 2) n doubles.  Traits are independent, so the batches change no bit of any result.
//
// The budget.  AQ_FM_STATE_BUDGET bounds the state (alpha and mu) of a batch.  batch_tiles = budget / (the state of the tile
// with the most work items), at least 1 and at most the number of tiles: every run of batch_tiles consecutive tiles then fits,
// whichever they are, and batch b is the tiles [b batch_tiles, (b + 1) batch_tiles).  4 GiB, chosen and not measured: at
// n = 500, windows of 5 000 predictors and L = 10 a tile has about 80 items and 52 MB of state, so a batch is about 80 tiles,
// 5 000 traits and 6 400 work items -- a dozen rounds of the 512 workgroups of the tile kernel that 256 CUs hold at a time,
// so that the ragged last round costs little -- while the state, the band buffer (a twentieth of it) and the fits
// (0.25 GB there) stay a small part of the device's memory next to the handle's own X.  A single tile above the budget still
// runs, alone.
#pragma once
#include "aq_cis_plan.h"

#define AQ_FM_LMAX 16
#define AQ_FM_STATE_BUDGET (4ll << 30)
#define AQ_FM_SAMPLE_BLOCK 64              // samples per workgroup of aq_k_fm_fit
#define AQ_FM_PURITY_MAX 100               // members of a credible set that aq_k_fm_purity looks at

// bytes of alpha and mu of one work item for L effects
static inline long long aq_fm_item_state_bytes(int L) { return 2ll * L * AQ_CIS_TILE * AQ_CIS_TILE * 8; }

// force_tiles: AQ_FM_BATCH_TILES (> 0), 0 when it is not set, < 0 when it is set but no number >= 1.  work may be NULL.
static inline int aq_finemap_make_plan(int n, int p1, int q, int ncu, const int32_t *s_lo, const int32_t *s_hi, int L, int force_tiles,
                                       const char *who, aq_finemap_plan *pl, aq_cis_work *work, std::string *err) {
  const std::string w(who);
  if (L < 1 || L > AQ_FM_LMAX) {
    if (err) *err = w + ": L must lie in [1, " + std::to_string(AQ_FM_LMAX) + "], " + std::to_string(L) + " given";
    return AQ_ERR_ARG;
  }
  if (force_tiles < 0) {
    if (err) *err = w + ": AQ_FM_BATCH_TILES must be a whole number >= 1";
    return AQ_ERR_ARG;
  }
  aq_cis_work local;
  aq_cis_work &wk = work ? *work : local;
  const int rc = aq_cis_make_plan(n, p1, q, 0, ncu, s_lo, s_hi, 0, 0, 0, who, &pl->cis, &wk, err);
  if (rc != AQ_OK) return rc;
  const int tiles = pl->cis.trait_tiles;
  long long most = 0;                       // the work items of the largest tile
  for (int k = 0; k < tiles; k++) most = std::max(most, (long long)wk.first_item[(size_t)k + 1] - wk.first_item[(size_t)k]);
  long long bt = 0;
  if (tiles > 0) {
    bt = force_tiles > 0 ? force_tiles : std::max(1ll, AQ_FM_STATE_BUDGET / std::max(1ll, most * aq_fm_item_state_bytes(L)));
    bt = std::min(bt, (long long)tiles);
  }
  long long items_most = 0, traits_most = 0;   // of one batch
  for (long long k0 = 0; k0 < tiles; k0 += bt) {
    const long long k1 = std::min((long long)tiles, k0 + bt);
    items_most = std::max(items_most, (long long)wk.first_item[(size_t)k1] - wk.first_item[(size_t)k0]);
    traits_most = std::max(traits_most, std::min((long long)pl->cis.q_active, k1 * AQ_CIS_TILE) - k0 * AQ_CIS_TILE);
  }
  pl->L = L;
  pl->batch_tiles = (int32_t)bt;
  pl->n_batches = bt > 0 ? (int32_t)((tiles + bt - 1) / bt) : 0;
  pl->forced = force_tiles > 0 ? 1 : 0;
  pl->state_budget = AQ_FM_STATE_BUDGET;
  pl->state_bytes = items_most * aq_fm_item_state_bytes(L);
  pl->band_bytes = items_most * AQ_CIS_TILE * AQ_CIS_TILE * 8;
  pl->fit_bytes = (long long)(L + 2) * traits_most * n * 8;
  return AQ_OK;
}
