// aq_plan.h -- the launch planner: which sweep kernel serves a problem and with what geometry.  A pure function of the problem
// sizes, the missingness counts, the device's CU count and memory, and the AQ_* hooks: integer and double arithmetic only, no
// HIP header, no device code, no getenv.  aq_vb_create (aq_vb_create.hip) runs it before it allocates anything; aq_plan_query
// exposes it on the C ABI without a device.  This is the single place where kernel and geometry are chosen.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

#include "../../include/atlasqtl_hip.h"
#include "aq_plan_const.h"

struct AqPlanInput {
  int n = 0, p = 0, q = 0;
  bool has_missing = false;      // Y holds at least one NaN
  int max_missing = 0;           // most missing samples of one trait
  int max_short_list = 0;        // largest over traits of min(missing, observed): the wide split's index lists (Mmax)
  int ncu = 256;                 // compute units of the device
  long long total_bytes = -1;    // the device's total memory; < 0 = unknown (only the wide split cannot do without it) ...
  const char *mem_error = nullptr;   // ... and why, for the message
};

struct AqPlan {
  bool use_la = false;   // look-ahead kernel (aq_core_sweep_la.h)
  bool use_mis = false;  // masked blocked MFMA kernel (aq_core_sweep_mis.h): missing Y, n <= 2048
  bool use_tw = false;   // generic wave-per-trait kernel (aq_trait_wave.h): missing Y, or n beyond the MFMA kernels
  bool la_mask = false;  // look-ahead kernel, MASK instances: Y with missing values, per-trait Gram blocks precomputed into GK
  bool la_wide = false;  // look-ahead kernel, wide sample split (9 <= laC <= AQ_LA_CMAX; n > 10240 or AQ_LA_C >= 9)
  int NT = 0;            // residual tiles of matrix waves 0,1,2 (look-ahead kernel) / per wave (masked kernel)
  int NT2 = 0;           // look-ahead kernel: tiles of matrix waves 4,5,6 (NT: waves 0,1,2)
  int NT3x = -1;         // look-ahead kernel, two-tile instances: 9 residual tiles on the recurrence wave (geometry NT / NT / 9), -1 = aq_la_nt3
  int TT = 1;            // look-ahead kernel: 16-trait tiles per workgroup (2 when there are enough tiles to fill the chip)
  int laC = 1;           // look-ahead kernel: workgroups (sample parts) per trait group, n > 1056
  int misC = 1;          // masked kernel: workgroups (sample parts) per trait tile
  int chain = 0;         // > 1: chained-segment launch with that many SNP segments (aq_core_sweep_la.h, SEG)
  int stagger = 0;       // look-ahead kernel: tile at which a matrix wave releases its SIMD partner into the phase (0 = off)
  int la_xhelper = 0;    // sample split of the look-ahead kernel: exchange on the helper wave (long matrix phases) or on the recurrence wave
  int la_xtouch = 1;     // helper waves warm the L2 with the next phase's X operand panels (AQ_XTOUCH=0 switches it off)
  int la_hprio = 0;      // s_setprio level of the helper wave (AQ_HPRIO; 1 for the unsplit MASK instances, see aq_plan_la)
  int la_mprio = 1;      // matrix waves: hand-offs at raised priority (AQ_MPRIO=0 switches it off): C3 34.84 -> 34.67 ms, C3 + 5 % NA 49.9 -> 47.1
  int NE = 0;            // samples per lane of the generic kernel
  int WPT = 1;           // generic kernel: waves (and workgroups) sharing one trait (tile); also rowGB rows per tile
  int tw_ns = 4;         // generic kernel: SNP columns staged in LDS at a time
  int Mmax = 0, NR = 0;  // longest per-trait index list (padded to 16); rows of the row-major SNP panels XR
  int p_pad = 0, q_pad = 0, n_pad = 0, nb = 0, ntile = 0;
  int ncu = 256;         // CU count the plan was made for (AQ_NCU)
};

// Lookup of an AQ_* hook by name: nullptr = not set.  aq_vb_create passes one that reads the environment and records what it
// found (aq_vb_get_overrides), aq_plan_query one that reads its overrides argument.  The planner never calls getenv itself.
using AqEnv = std::function<const char *(const char *)>;

// The hooks (tests and experiments).  Deliberately NOT all read up front: each is looked up and parsed once, when the planner
// first comes to the decision it overrides, because a handle reports exactly the hooks its plan consulted, in that order
// (aq_vb_get_overrides), and a hook of a path not taken was never among them.  The cost models test these fields, not strings.
// An empty AqEnv means "no hook is set".
enum AqHook { AQ_H_NCU, AQ_H_KERNEL, AQ_H_LA_C, AQ_H_GK_MAX_GB, AQ_H_MIS_C, AQ_H_TW_WPT, AQ_H_TT, AQ_H_NT3, AQ_H_LA_NOSPLIT,
              AQ_H_LA_XHELPER, AQ_H_XTOUCH, AQ_H_MPRIO, AQ_H_HPRIO, AQ_H_STAGGER, AQ_H_CHAIN, AQ_H_COUNT };
static const char *const aq_hook_names[AQ_H_COUNT] = {"AQ_NCU", "AQ_KERNEL", "AQ_LA_C", "AQ_GK_MAX_GB", "AQ_MIS_C", "AQ_TW_WPT", "AQ_TT", "AQ_NT3",
                                                      "AQ_LA_NOSPLIT", "AQ_LA_XHELPER", "AQ_XTOUCH", "AQ_MPRIO", "AQ_HPRIO", "AQ_STAGGER", "AQ_CHAIN"};
struct AqOpt { bool set = false, seen = false; int v = 0; double d = 0.0; };   // v, d: atoi, atof of the value
struct AqHooks {
  const AqEnv &env;
  AqOpt opt[AQ_H_COUNT];
  const AqOpt &operator[](AqHook h) {
    AqOpt &o = opt[h];
    if (!o.seen) {
      o.seen = true;
      if (const char *v = env ? env(aq_hook_names[h]) : nullptr) { o.set = true; o.v = atoi(v); o.d = atof(v); }
    }
    return o;
  }
};

static inline int aq_plan_fail(std::string *err, int code, const std::string &msg) {
  if (err) *err = msg;
  return code;
}
static inline int aq_round16(int x) { return (x + 15) / 16 * 16; }

// ---- memory budget 1: do the per-trait Gram blocks of the MASK instances fit? ------------------------------------------------
// Y with missing values: the look-ahead kernel's MASK instances when the per-trait Gram blocks (50 KB per trait tile and
// SNP block, computed once) fit next to the rest of the state in HBM; else the masked two-barrier kernel (AQ_KERNEL=3
// forces that one), which recomputes them every sweep.
static inline int aq_plan_gk_budget(const AqPlanInput &in, AqHooks &h, bool wide, bool *la_mask_ok, std::string *err) {
  const size_t ntile_ = (size_t)(in.q + 15) / 16, nb_ = (size_t)(in.p + 15) / 16;
  const size_t gk_b = ntile_ * nb_ * AQ_GK_STRIDE * sizeof(double);
  const size_t rest_b = 2 * ntile_ * nb_ * 256 * sizeof(double) + 3 * (size_t)(in.n + 64) * nb_ * 16 * sizeof(double) * 2 +
                        3 * ntile_ * (size_t)(in.n + 64) * 16 * sizeof(double);
  // decided on the device's TOTAL memory (minus a tenth), not on what happens to be free: the same problem gets the same
  // kernel on every rank and in every run, so a checkpoint of one is accepted by the other.  Should the allocation then fail
  // because other processes hold memory, aq_vb_create reports the out-of-memory error (AQ_GK_MAX_GB lowers the limit).
  const bool mem_known = in.total_bytes >= 0;
  if (wide && !mem_known) return aq_plan_fail(err, AQ_ERR_DEVICE, std::string("hipMemGetInfo: ") + (in.mem_error ? in.mem_error : "failed"));
  // (the wide split sizes its whole budget, with its own n_pad, before allocating: see aq_plan_wide_budget)
  if (!mem_known || (!wide && (double)(gk_b + rest_b) * 1.05 > 0.9 * (double)in.total_bytes)) *la_mask_ok = false;
  const AqOpt &e = h[AQ_H_GK_MAX_GB];
  if (e.set && (double)gk_b > e.d * 1e9) *la_mask_ok = false;   // test hook: force the fallback
  if (wide && !*la_mask_ok) {   // AQ_GK_MAX_GB: no fallback kernel at this n
    char msg[256];
    snprintf(msg, sizeof msg, "Y with missing values at n = %d: the per-trait Gram blocks need %.1f GB of device memory, which does not "
             "fit; shard the traits (fewer traits per device)", in.n, (double)gk_b / 1e9);
    return aq_plan_fail(err, AQ_ERR_UNSUPPORTED, msg);
  }
  return AQ_OK;
}

// ---- kernel choice ------------------------------------------------------------------------------------------------------------
// default: look-ahead kernel (complete Y, n <= 1056); AQ_KERNEL=2 forces the generic wave-per-trait kernel
// missing values: masked blocked MFMA kernel while n fits 8 waves x 16 residual tiles and no trait misses more
// than AQ_MIS_MMAX samples; otherwise (and with AQ_KERNEL=2) the generic kernel
// the masked MFMA kernel also serves complete Y beyond the look-ahead kernel's n (all-ones mask, empty lists)
// Complete Y beyond n = 1056: look-ahead kernel with a sample split.
static inline int aq_plan_kernel(const AqPlanInput &in, AqHooks &h, AqPlan *pl, bool *wide_out, std::string *err) {
  const AqOpt &ek = h[AQ_H_KERNEL];
  const bool n_la_ok = in.n <= 8 * 16 * 105;
  // n > 10240 (or AQ_LA_C = 9 ... AQ_LA_CMAX, test hook): the look-ahead kernel's wide sample split, complete Y or MASK with the
  // Gram blocks of aq_k_gk_blocks_g (any missingness); no other kernel serves this n
  const AqOpt &ecw = h[AQ_H_LA_C];
  const bool wide = in.n > 10240 || (ecw.set && ecw.v >= 9);
  if (wide && ecw.set && (ecw.v > AQ_LA_CMAX || (in.n > 10240 && ecw.v < 9)))
    return aq_plan_fail(err, AQ_ERR_ARG, "AQ_LA_C: the wide sample split takes 9 ... " + std::to_string(AQ_LA_CMAX) + " parts");
  if (wide && ek.set && ek.v >= 2) return aq_plan_fail(err, AQ_ERR_UNSUPPORTED, "AQ_KERNEL: only the look-ahead kernel serves n > 10240");
  bool la_mask_ok = in.has_missing && n_la_ok && in.max_missing <= AQ_MIS_MMAX && !(ek.set && ek.v >= 2);
  if (wide) la_mask_ok = in.has_missing;
  if (la_mask_ok) {
    const int rc = aq_plan_gk_budget(in, h, wide, &la_mask_ok, err);
    if (rc != AQ_OK) return rc;
  }
  const bool la_split_ok = (!in.has_missing && in.n > 1056 && n_la_ok && !(ek.set && ek.v >= 2)) || (wide && !in.has_missing);   // complete Y, large n
  if (!wide && !la_mask_ok && (in.has_missing || (in.n > 1056 && !la_split_ok)) && in.n <= 16384 && in.max_missing <= AQ_MIS_MMAX && !(ek.set && ek.v == 2))
    pl->use_mis = true;
  else if (!wide && ((in.has_missing && !la_mask_ok) || (ek.set && ek.v == 2) || (in.n > 1056 && !la_split_ok && !la_mask_ok)))
    pl->use_tw = true;
  else {
    pl->use_la = true;
    pl->la_mask = la_mask_ok;
  }
  *wide_out = wide;
  return AQ_OK;
}

// ---- chained segments, both MFMA kernels --------------------------------------------------------------------------------------
// more workgroups than CUs: chained SNP segments even out the last round (3 rounds -> ~2.5 for 625 workgroups).  nwg trait
// groups of nb SNP blocks; split: the parts of a group must be co-resident, so no chained segments.
static inline int aq_plan_chain(AqHooks &h, bool mis, int nwg, int nb, int ncu, bool split) {
  int chain = 0;
  auto rounds = [&](long long wg) { return (double)((wg + ncu - 1) / ncu); };
  if (nwg > ncu && !split) {
    // look-ahead kernel: cost of a sweep in phases: rounds of workgroups x (SNP blocks of a segment + 2 phases of pipeline fill +
    // ~1.7 of start-up: fitted to C3 at S = 4, 8, 13, 16, 26, profiles/r03_chain_segments.txt).  C3: 313 groups -> S = 13 (16 rounds
    // of 241 blocks: 34.43 ms against 34.61 with S = 4); C3 with NA: 625 groups -> S = 9.
    // masked kernel: rounds per segment with 0.2 % of a sweep per further segment, S <= 16.
    double best = 1e30;
    const int smax = mis ? 16 : std::min(32, nb);
    for (int S = 2; S <= smax; S++) {
      const double cost = mis ? rounds((long long)nwg * S) / S * (1.0 + 0.002 * S) : rounds((long long)nwg * S) * ((nb + S - 1) / S + 3.7);
      if (cost < best - (mis ? 1e-12 : 1e-9)) { best = cost; chain = S; }
    }
    if (best >= (mis ? rounds(nwg) : rounds(nwg) * (nb + 3.7))) chain = 0;   // no gain over whole tiles
  }
  const AqOpt &e = h[AQ_H_CHAIN];
  if (e.set) chain = e.v > 1 ? e.v : 0;
  if (chain > nb) chain = nb;
  if (chain > 32) chain = 32;
  if (split) chain = 0;
  return chain;
}

// ---- masked kernel geometry ---------------------------------------------------------------------------------------------------
static inline void aq_plan_mis(const AqPlanInput &in, AqHooks &h, AqPlan *pl) {
  // n_pad = 128 NT C: C workgroups per trait tile, NT in AQ_MIS_NT residual tiles per wave.  Model of a sweep:
  // whole rounds of workgroups (one per CU) x time per SNP block (4.5 + 0.94 NT us, + 6 us for the exchange)
  {
    const int ntile_ = (in.q + 15) / 16;
    double best = 1e300;
    for (int C = 1; C <= 8; C++)
      for (int NT : AQ_MIS_NT) {
        if (128 * NT * C < in.n) continue;
        double rounds = (double)(((long long)ntile_ * C + pl->ncu - 1) / pl->ncu);
        double cost = rounds * (4.5 + 0.94 * NT + (C > 1 ? 6.0 : 0.0));
        if (cost < best - 1e-9) { best = cost; pl->misC = C; pl->NT = NT; }
      }
  }
  const AqOpt &e = h[AQ_H_MIS_C];   // test hook: force the sample split at small n
  if (e.set && e.v >= 1 && e.v <= 8) {
    pl->misC = e.v;
    constexpr int NNT = sizeof AQ_MIS_NT / sizeof *AQ_MIS_NT;
    pl->NT = AQ_MIS_NT[NNT - 1];
    for (int i = NNT - 1; i >= 0; i--) if (128 * AQ_MIS_NT[i] * e.v >= in.n) pl->NT = AQ_MIS_NT[i];
  }
  pl->Mmax = std::max(16, aq_round16(in.max_missing));
  if (pl->misC == 1) pl->chain = aq_plan_chain(h, true, pl->ntile, pl->nb, pl->ncu, false);   // same chained-segment choice as for the look-ahead kernel
  pl->n_pad = 128 * pl->NT * pl->misC;
  pl->NR = pl->n_pad + 8;
}

// ---- generic kernel geometry: n_pad = 64 * NE * WPT samples, WPT waves (and workgroups) per trait (tile) ----------------------
static inline void aq_plan_tw(const AqPlanInput &in, AqHooks &h, AqPlan *pl) {
  // the fewest waves whose largest instance holds n (n <= 2048: 1, n <= 5120: 2), else the most; then the smallest NE that does
  constexpr int NNE = sizeof AQ_TW_NE / sizeof *AQ_TW_NE, NWPT = sizeof AQ_TW_WPT / sizeof *AQ_TW_WPT;
  pl->WPT = AQ_TW_WPT[NWPT - 1];
  for (int i = NWPT - 1; i >= 0; i--) if (in.n <= 64 * aq_tw_ne_max(AQ_TW_WPT[i]) * AQ_TW_WPT[i]) pl->WPT = AQ_TW_WPT[i];
  const AqOpt &e = h[AQ_H_TW_WPT];   // test hook
  if (e.set && aq_tw_built(AQ_TW_NE[0], e.v) && e.v > pl->WPT) pl->WPT = e.v;
  const int per_lane = (in.n + 64 * pl->WPT - 1) / (64 * pl->WPT);
  pl->NE = AQ_TW_NE[NNE - 1];
  for (int i = NNE - 1; i >= 0; i--) if (per_lane <= AQ_TW_NE[i]) pl->NE = AQ_TW_NE[i];
  pl->n_pad = 64 * pl->NE * pl->WPT;
  // SNP columns staged in LDS at a time: ns * n_pad doubles next to 18 KB of block scalars, within 160 KB
  pl->tw_ns = 4;
  while (pl->tw_ns > 1 && (size_t)(pl->tw_ns * pl->n_pad + 8 * 256 + 32) * sizeof(double) > 150 * 1024) pl->tw_ns /= 2;
}

// ---- look-ahead kernel geometry -----------------------------------------------------------------------------------------------
// 6 matrix waves (NT tiles on waves 0-2, NT2 = NT or NT - 1 on waves 4-6: NT + NT2 per SIMD) + the recurrence wave,
// which owns aq_la_nt3(NT, TT) tiles of its own when two trait tiles share a workgroup.
// aq_la_fit: smallest geometry that holds tiles_needed: NT in 1..nt_max (AQ_LA_NT_UNSPLIT or, for a sample split, AQ_LA_NT_SPLIT: the
// instance set of aq_plan_const.h), NT2 in {NT, NT - 1}, plus the recurrence wave's aq_la_nt3
// tiles; among equals the one with more tiles on the recurrence wave (AQ_NT3=0/3/6 pins its tile count for experiments).
// Returns the tile count, 1 << 30 when nothing fits.
static inline int aq_la_fit(int TT, bool la_mask, const AqOpt &e3, int tiles_needed, int nt_max, int *NTo, int *NT2o, int *N3xo) {
  int best_tiles = 1 << 30, best_nt3 = -1;
  for (int NT = 1; NT <= nt_max; NT++)
    for (int NT2 = NT; NT2 >= (NT > 1 ? NT - 1 : NT); NT2--) {
      // x9: the instance NT / NT / 9 -- nine residual tiles on the recurrence wave, 18 instead of 19 per matrix SIMD at
      // n = 1000.  While the recurrence wave's MFMAs hold SIMD 3's datapath the helper wave's fp64 work crawls (38.4 ms at C3
      // against 34.3 for 10 / 9 / 6), so it comes with the helper wave one priority level up (aq_plan_la): 33.9 ms
      // (profiles/r03_nt9_stagger.txt).  AQ_NT3 pins another count; the diagnostic build, whose NT / NT / 9 instances do not
      // pass the ISA proof and are not built (AQ_LA_TT2_REC9, aq_plan_const.h), takes it only on request.
      // (by default from NT = 9 on: 8 / 8 / 9 -- n around 900 -- loses to 9 / 8 / 6, 8.68 against 8.42 us per phase; measured per
      // geometry in profiles/r03_nt9_stagger.txt: a phase takes max(matrix SIMDs, SIMD 3) with SIMD 3 at 7.6 - 7.7 us for three or
      // six tiles and 8.7 for nine, the matrix SIMDs at 7.6 / 7.7 / 8.4 / 8.4 / 8.9 / 9.3 / 9.7 / 10.3 us for (8,7) ... (11,11))
      const bool x9_ok = TT == 2 && NT2 == NT && (e3.set ? (NT >= AQ_LA_NT_REC && e3.v == 9) : (AQ_LA_TT2_REC9 && NT >= 9));
      for (int x9 = 0; x9 <= (x9_ok ? 1 : 0); x9++) {
        int nt3 = x9 ? 9 : aq_la_nt3(NT, NT2, TT);
        // one tile per workgroup, unsplit (the trait shards of N = 2, 4: MFMA-bound on three SIMDs while SIMD 3 only runs
        // the chain): three residual tiles on the recurrence wave by default -- q = 5000: 19.55 -> 18.78 ms, q = 2500:
        // 15.48 -> 14.83; six or nine make its chain + tiles the bound (30 and 33 ms).  AQ_NT3 = 0 / 3 / 6 / 9 pins the count.
        int x1 = -1;
        bool second = false;
        if (TT == 1 && !la_mask && NT >= AQ_LA_NT_REC && nt_max <= AQ_LA_NT_UNSPLIT) {
          const int w = e3.set ? e3.v : 3;
          if ((w == 3 || w == 6 || w == 9) && NT2 == aq_la_rec_nt2(NT, w)) x1 = w;
          else if (e3.set && w != 0) continue;
          if (x1 > 0) nt3 = x1;
          second = !e3.set && x1 > 0;        // by default the plain geometry competes as well (it wins when it needs fewer tiles)
        }
        if (second) {
          const int tiles0 = 3 * (NT + NT2);
          if (tiles0 >= tiles_needed && tiles0 < best_tiles) { best_tiles = tiles0; best_nt3 = 0; *NTo = NT; *NT2o = NT2; *N3xo = -1; }
        }
        const int tiles = 3 * (NT + NT2) + nt3;
        if (tiles < tiles_needed || (e3.set && e3.v != nt3 && TT == 2 && NT >= AQ_LA_NT_REC)) continue;
        if (tiles < best_tiles || (tiles == best_tiles && nt3 > best_nt3)) { best_tiles = tiles; best_nt3 = nt3; *NTo = NT; *NT2o = NT2; *N3xo = x9 ? 9 : x1; }
      }
    }
  return best_tiles;
}

// n <= 1056: one workgroup per trait group holds all samples; with few trait groups the idle CUs share them
static inline int aq_plan_la_unsplit(AqHooks &h, AqPlan *pl, const AqOpt &e3, int ntiles, std::string *err) {
  pl->laC = 1;
  const int tiles = aq_la_fit(pl->TT, pl->la_mask, e3, ntiles, AQ_LA_NT_UNSPLIT, &pl->NT, &pl->NT2, &pl->NT3x);    // n <= 1056 always fits (11, 11) ...
  if (tiles >= (1 << 30)) return aq_plan_fail(err, AQ_ERR_ARG, "AQ_NT3 excludes every look-ahead geometry for this n");   // ... unless the test hook forbids it
  pl->n_pad = 16 * tiles;
  // Few trait groups (a trait shard of a multi-GPU run, a small q): the CUs left idle share the samples.  Per SNP block an
  // unsplit workgroup needs its MFMA stream (0.213 us per residual tile of one SIMD + 1.0 of hand-offs; n = 1000: 5.46 us
  // measured) or, for small n, the chain (3.3 us); a part of a split group needs its shorter stream or chain + exchange
  // (4.5 us with two parts, measured at n = 1000: 4.53; + 0.2 per further part).  All parts must run at once.
  // (Not with missing values: there the chain is longer and the helper wave loaded -- q = 1250 with 5 % NA: 19.3 ms unsplit,
  // 20.1 split.  AQ_LA_NOSPLIT=1 keeps one workgroup per group: experiments.)
  if (pl->TT == 1 && !pl->la_mask && !h[AQ_H_LA_NOSPLIT].set) {
    double best = std::max(0.213 * (pl->NT + pl->NT2) + 1.0, 3.3) * 0.95;   // a split must win by 5 %
    for (int C = 2; C <= 8 && (long long)pl->ntile * C <= pl->ncu; C++) {
      int NT = 0, NT2 = 0, N3x = -1;
      const int tiles_c = aq_la_fit(pl->TT, pl->la_mask, e3, (ntiles + C - 1) / C, AQ_LA_NT_SPLIT, &NT, &NT2, &N3x);
      if (tiles_c >= (1 << 30)) continue;
      const double cost = std::max(0.213 * (NT + NT2) + 1.0, 4.5 + 0.2 * (C - 2));
      if (cost < best - 1e-9) { best = cost; pl->laC = C; pl->NT = NT; pl->NT2 = NT2; pl->NT3x = N3x; pl->n_pad = 16 * tiles_c * C; }
    }
  }
  return AQ_OK;
}

// n beyond one workgroup's registers: C workgroups share a trait group (sample split, one tile per workgroup).  Cost of
// a sweep ~ rounds of workgroups x time per SNP block: the MFMA stream of one SIMD (0.213 us per residual tile) or the
// exchange + chain (4.5 us with two parts, + 0.2 per further part), whichever is longer.  (AQ_LA_C forces the split at small n: test hook.)
// Returns the cost of the best plan, 1e300 when there is none.
static inline double aq_plan_la_medium(AqPlan *pl, const AqOpt &e3, const AqOpt &ec, int ntiles) {
  double best = 1e300;
  for (int C = 2; C <= 8; C++) {
    if (ec.set && ec.v != C) continue;
    int NT = 0, NT2 = 0, N3x = -1;
    const int tiles = aq_la_fit(pl->TT, pl->la_mask, e3, (ntiles + C - 1) / C, AQ_LA_NT_SPLIT, &NT, &NT2, &N3x);
    if (tiles >= (1 << 30)) continue;
    const double rounds = (double)(((long long)pl->ntile * C + pl->ncu - 1) / pl->ncu);
    const double cost = rounds * std::max(0.213 * (NT + NT2) + 1.0, 4.5 + 0.2 * (C - 2));
    if (cost < best - 1e-9) { best = cost; pl->laC = C; pl->NT = NT; pl->NT2 = NT2; pl->NT3x = N3x; pl->n_pad = 16 * tiles * C; }
  }
  return best;
}

// the wide split (aq_launch_la1w.hip): C = 9 ... AQ_LA_CMAX parts of 6 NT residual tiles (NT2 = NT, none on the recurrence
// wave), the exchange a block ahead on the helper wave.  Same model: rounds of workgroups x time per SNP block, here
// max(MFMA stream of one SIMD, helper wave), because the exchange runs on the helper wave next to its own per-block work
// (staging, column sums) and adds to it.  Measured (timelines of workgroup 0, profiles/large_n_timeline.txt, n = 20 480):
// helper period 8.5 us at C = 12, 10.9 us at C = 29 (exchange 3.7 -> 6.3 us, the rest 4.6 - 4.9 us) -> 8.5 + 0.14 (C - 12).
// (Not modelled: at n = 50 000 the operand stream of the matrix waves and the exchange are both slower)
static inline double aq_plan_la_wide(AqPlan *pl, const AqOpt &ec, int ntiles) {
  auto helper_us = [](int C) { return 8.5 + 0.14 * (C - 12); };
  double best = 1e300;
  pl->la_wide = true;
  const int cf = ec.set ? ec.v : 0;
  for (int C = 9; C <= AQ_LA_CMAX && C <= pl->ncu; C++) {
    if (cf >= 9 && C != cf) continue;
    const int NT = ((ntiles + C - 1) / C + 5) / 6;
    if (NT > AQ_LA_NT_WIDE) continue;
    const double rounds = (double)(((long long)pl->ntile * C + pl->ncu - 1) / pl->ncu);
    const double cost = rounds * std::max(0.213 * 2 * NT + 1.0, helper_us(C));
    if (cost < best - 1e-9) { best = cost; pl->laC = C; pl->NT = NT; pl->NT2 = NT; pl->NT3x = -1; pl->n_pad = 16 * 6 * NT * C; }
  }
  return best;
}

static inline int aq_plan_la(const AqPlanInput &in, AqHooks &h, bool wide, AqPlan *pl, std::string *err) {
  const int ntiles = (in.n + 15) / 16;
  const bool split = !(in.n <= 1056 && !h[AQ_H_LA_C].set);
  // two trait tiles per workgroup once that still gives every CU a workgroup (C3: 625 tiles -> 313 workgroups of 32
  // traits): X operands shared by two MFMAs, one chain evaluation per 32 traits, half the per-phase overhead.
  // q is then padded to a multiple of 32 (the extra tile is all padding: zero residual, masked sums).
  // (Crossover measured at n = 1000, 256 CUs: 448 tiles -- one round of two-tile workgroups, 27.4 ms, against 1.75 rounds of
  // one-tile workgroups; q = 8000: 27.5 vs 31.1 ms, q = 6144: 27.5 vs 23.4.)
  pl->TT = (4LL * pl->ntile >= 7LL * pl->ncu) ? 2 : 1;
  const AqOpt &ett = h[AQ_H_TT];
  if (ett.set) pl->TT = ett.v == 2 ? 2 : 1;
  if (pl->la_mask) pl->TT = 1;   // 16 per-trait Gram blocks per trait tile in LDS: one tile per workgroup
  if (split) pl->TT = 1;         // sample split: one tile per workgroup
  if (pl->TT == 2) {
    pl->q_pad = (in.q + 31) / 32 * 32;
    pl->ntile = pl->q_pad / 16;
    // (waves 4-6 then enter a phase when their SIMD partner is a third of the way through it -- stagger, set below -- so
    // that one wave's hand-off gap is covered by the other's MFMAs)
  }
  const AqOpt &e3 = h[AQ_H_NT3];
  if (!split) {
    const int rc = aq_plan_la_unsplit(h, pl, e3, ntiles, err);
    if (rc != AQ_OK) return rc;
  } else {
    const AqOpt &ec = h[AQ_H_LA_C];
    const double best = wide ? aq_plan_la_wide(pl, ec, ntiles) : aq_plan_la_medium(pl, e3, ec, ntiles);
    if (best >= 1e300) return aq_plan_fail(err, AQ_ERR_UNSUPPORTED, "no look-ahead geometry for this n");
    // Who exchanges the partial S': the recurrence wave at the start of its chain.  The helper wave can do it a block ahead
    // (AQ_LA_XHELPER=1); that paid at n = 5000 while an exchange was three trips through the shared cache (236 vs 225 ms),
    // with self-validating words it no longer does (222.5 vs 222.0; n = 1500: 58.3 vs 64.5).  The wide split's exchange runs
    // on the helper wave.
    pl->la_xhelper = wide ? 1 : 0;
  }
  if (h[AQ_H_LA_XHELPER].set) pl->la_xhelper = h[AQ_H_LA_XHELPER].v != 0;   // test hook
  if (h[AQ_H_XTOUCH].set) pl->la_xtouch = h[AQ_H_XTOUCH].v != 0;
  // helper wave one priority level above the recurrence wave it shares SIMD 3 with -- only where its iteration is on the
  // critical cycle: the unsplit MASK instances (single cross-block buffer; C3 + 5 % NA 49.9 -> 48.6 ms on one box, 48.4 -> 47.4
  // on another; the split C5 shard 241.1 -> 242.0, complete Y the same within noise: profiles/r03_hprio_na.txt)
  if (pl->la_mask && pl->laC <= 1) pl->la_hprio = 1;
  // six or nine tiles on the recurrence wave of a two-tile workgroup: see aq_la_fit (n = 800, geometry 8 / 7 / 6: 33.5 -> 29.6 ms)
  if (pl->TT == 2 && pl->NT >= AQ_LA_NT_REC && (pl->NT3x == 9 || (pl->NT3x < 0 && pl->NT2 == pl->NT - 1))) pl->la_hprio = 1;
  if (h[AQ_H_MPRIO].set) pl->la_mprio = h[AQ_H_MPRIO].v != 0;
  const AqOpt &ehp = h[AQ_H_HPRIO];
  if (ehp.set) pl->la_hprio = ehp.v >= 0 && ehp.v <= 3 ? ehp.v : 0;
  if (pl->TT == 2) pl->stagger = (pl->NT + 2) / 3;
  const AqOpt &est = h[AQ_H_STAGGER];
  if (est.set) pl->stagger = est.v >= 0 ? est.v : 0;
  pl->chain = aq_plan_chain(h, false, pl->ntile / pl->TT, pl->nb, pl->ncu, pl->laC > 1);
  // the index lists of the MASK instances: per trait its missing samples -- wide split: the shorter of the missing and the
  // observed list (aq_k_gk_blocks_g)
  if (pl->la_wide) pl->Mmax = pl->la_mask ? aq_round16(in.max_short_list) : 0;
  else if (pl->la_mask) pl->Mmax = aq_round16(in.max_missing);
  if ((pl->la_wide || pl->la_mask) && pl->Mmax < 16) pl->Mmax = 16;
  if (pl->la_mask) pl->NR = pl->n_pad + 8;
  return AQ_OK;
}

// ---- memory budget 2: device memory of the wide split -------------------------------------------------------------------------
// the X operand panels (XA, XU: n_pad p 8 B each), residual and mask tiles, and with missing values the Gram blocks plus,
// while they are built, the row panels XR and the index lists.  No other kernel serves this n: fail here, before anything
// is allocated, when it cannot fit.
static inline int aq_plan_wide_budget(const AqPlanInput &in, const AqPlan &pl, std::string *err) {
  const double xb = 2.0 * (double)pl.nb * (pl.n_pad / 16) * 128 * sizeof(double);
  const double rb = (pl.la_mask ? 2.0 : 1.0) * (double)pl.ntile * pl.n_pad * 16 * sizeof(double);
  const double gb = pl.la_mask ? (double)pl.ntile * pl.nb * AQ_GK_STRIDE * sizeof(double) + (double)pl.nb * (pl.n_pad + 8) * 16 * sizeof(double) +
                                     (double)pl.ntile * 16 * pl.Mmax * sizeof(int)
                               : 0.0;
  if (in.total_bytes < 0) return aq_plan_fail(err, AQ_ERR_DEVICE, "hipMemGetInfo failed");
  if ((xb + rb + gb) * 1.05 > 0.9 * (double)in.total_bytes) {
    char msg[256];
    snprintf(msg, sizeof msg, "n = %d, p = %d, q = %d: the wide sample split needs %.1f GB of device memory, more than the device holds; "
             "shard the traits (fewer traits per device)", in.n, in.p, in.q, (xb + rb + gb) * 1.05 / 1e9);
    return aq_plan_fail(err, AQ_ERR_UNSUPPORTED, msg);
  }
  return AQ_OK;
}

// ---- the planner --------------------------------------------------------------------------------------------------------------
static inline int aq_make_plan(const AqPlanInput &in, const AqEnv &env, AqPlan *out, std::string *err) {
  if (in.n > AQ_N_MAX)
    return aq_plan_fail(err, AQ_ERR_UNSUPPORTED, "n = " + std::to_string(in.n) + " exceeds the largest supported sample count, n <= " +
                                                     std::to_string(AQ_N_MAX) + " (AQ_N_MAX, the wide sample split)");
  AqHooks h{env, {}};
  AqPlan pl;
  pl.p_pad = aq_round16(in.p);
  pl.q_pad = aq_round16(in.q);
  pl.nb = pl.p_pad / 16;
  pl.ntile = pl.q_pad / 16;
  pl.ncu = in.ncu;
  if (h[AQ_H_NCU].set && h[AQ_H_NCU].v > 0) pl.ncu = h[AQ_H_NCU].v;
  bool wide = false;
  int rc = aq_plan_kernel(in, h, &pl, &wide, err);
  if (rc != AQ_OK) return rc;
  if (pl.use_mis) aq_plan_mis(in, h, &pl);
  else if (pl.use_tw) aq_plan_tw(in, h, &pl);
  else rc = aq_plan_la(in, h, wide, &pl, err);
  if (rc == AQ_OK && pl.la_wide) rc = aq_plan_wide_budget(in, pl, err);
  if (rc != AQ_OK) return rc;
  *out = pl;
  return AQ_OK;
}

// ---- the plan as aq_vb_status reports it (aq_vb_get_status and aq_plan_query) ------------------------------------------------
static inline int aq_core_kernel_id(const AqPlan &pl) { return pl.use_mis ? 3 : pl.use_tw ? 2 : 0; }
static inline void aq_plan_to_status(const AqPlan &pl, aq_vb_status *st) {
  st->core_kernel = aq_core_kernel_id(pl);
  st->split_parts = pl.use_la ? pl.laC : pl.use_mis ? pl.misC : 1;
  st->tiles_per_group = pl.use_la ? pl.TT : 1;
  st->chain_segments = pl.chain > 1 ? pl.chain : 0;
  // the instance aq_launch_core dispatches to (aq_launch_la.h): a wide instance has NT2 == NT and no tiles on the recurrence wave
  st->tiles_matrix = (pl.use_la || pl.use_mis) ? pl.NT : 0;
  st->tiles_matrix2 = pl.use_la ? pl.NT2 : 0;
  st->tiles_recurrence = (pl.use_la && !pl.la_wide) ? aq_la_rec_tiles(pl.NT, pl.NT2, pl.TT, pl.NT3x) : 0;
  st->instance_flags = pl.use_la ? (pl.la_mask ? 1 : 0) | (pl.la_wide ? 2 : 0) | (pl.chain > 1 ? 4 : 0) : 0;
  st->n_pad = pl.n_pad;
}
