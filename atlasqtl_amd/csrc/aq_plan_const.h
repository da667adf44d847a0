// aq_plan_const.h -- the geometry limits that the sweep kernels (aq_core_sweep.h, aq_core_sweep_mis.h) share with the host's
// launch planner (aq_plan.h).  Plain C++: no HIP header, no device code.
#pragma once

// Look-ahead kernel: 16-sample residual tiles owned by the RECURRENCE wave (on top of the 3 (NT + NT2) of the six matrix
// waves).  With two trait tiles per workgroup a phase is long enough for that wave to run its chain and then some matrix
// work on SIMD 3, which otherwise issues no MFMA at all.  Shared by the kernel template and the host's geometry.
constexpr int AQ_GK_DIAG = 136 * 16, AQ_GK_STRIDE = 136 * 16 + 256 * 16;   // doubles per (tile, SNP block) of AqCoreArgs::GK
// wide sample split of the look-ahead kernel (n > 10240): at most AQ_LA_CMAX parts per trait group, each holding at most 108
// residual tiles of 16 samples (NT = NT2 = 18 on six matrix waves, the largest instance), so n <= AQ_N_MAX = 48 x 108 x 16 =
// 82 944: the geometry is the limit (sample indices are int32 and every offset into R, mis and the X panels is 64-bit).
// AQ_LA_WPC: most partner words one lane of split_exchange_wide sums, ceil(C / floor(64 / ceil(256 / C))) -- checked below for
// every C the host can choose.
constexpr int AQ_LA_CMAX = 48, AQ_N_MAX = AQ_LA_CMAX * 108 * 16, AQ_LA_WPC = 6;
constexpr bool aq_la_wide_lanes_ok() {
  for (int C = 9; C <= AQ_LA_CMAX; C++) {
    const int cmax = (256 + C - 1) / C, nch = 64 / cmax, pc = (C + nch - 1) / nch;
    if (nch < 1 || nch * cmax > 64 || pc > AQ_LA_WPC) return false;
  }
  return true;
}
static_assert(aq_la_wide_lanes_ok(), "split_exchange_wide: some C in 9..AQ_LA_CMAX needs more than AQ_LA_WPC partner words per lane");
#define AQ_MIS_MMAX 1024  // most missing samples of one trait the LDS index lists hold (16-bit indices, padded to 16)

// ---- the compiled instance set of the three sweep kernels -------------------------------------------------------------------
// The one place that says which template instances exist.  The launch units (aq_launch_la*.hip, aq_vb_sweep.hip) instantiate
// exactly the parameters for which aq_la_built / aq_tw_built / aq_mis_built hold, the planner (aq_plan.h) searches within these
// limits, and aq_instance_query answers from the launchers' own walk over them.
//
// Look-ahead kernel aq_core_sweep_la_kernel<NT, NT2, SEG, TT, MASK, NT3_, WIDE>: NT2 is NT or NT - 1 (at least 1) throughout.
constexpr int AQ_LA_NT_UNSPLIT = 11;   // NT = 1 ... 11: the unsplit launches (n <= 1056), plain and chained (SEG), TT = 1 and 2
constexpr int AQ_LA_NT_SPLIT = 18;     // NT = 12 ... 18: the sample split of large n only, TT = 1 -- never chained: the parts of a
                                       // group must be co-resident
constexpr int AQ_LA_NT_REC = 8;        // from this NT on (to AQ_LA_NT_UNSPLIT) the recurrence wave can own residual tiles
constexpr int AQ_LA_NT_WIDE = 18;      // WIDE: NT = 1 ... 18 with NT2 == NT, TT = 1, unchained, no tiles on the recurrence wave
// The cycle counters of the diagnostic build push the TT = 2 NT / NT / 9 instances over the register budget (the ISA proof stops
// them): that build compiles none, and its planner takes the geometry only on request (aq_la_fit).
#ifdef AQ_DIAG_TIME
constexpr bool AQ_LA_TT2_REC9 = false;
#else
constexpr bool AQ_LA_TT2_REC9 = true;
#endif
// tiles of the recurrence wave where the instance names no count of its own (NT3_ = -1): two tiles per workgroup only
constexpr int aq_la_nt3(int NT, int NT2, int TT) { return (TT == 2 && NT >= AQ_LA_NT_REC) ? (NT2 == NT ? 3 : 6) : 0; }
// ... and of any instance or plan: NT3x as the planner holds it (-1 = aq_la_nt3's count) -> the count aq_vb_status reports
constexpr int aq_la_rec_tiles(int NT, int NT2, int TT, int NT3x) { return NT3x > 0 ? NT3x : aq_la_nt3(NT, NT2, TT); }
// the counts an instance can name, and the NT2 each goes with: 3: NT / NT, 6: NT / NT - 1, 9: NT / NT
constexpr int AQ_LA_REC_FORMS[] = {3, 6, 9};
constexpr int aq_la_rec_nt2(int NT, int rec) { return rec == 6 ? NT - 1 : NT; }
constexpr bool aq_la_built(int NT, int NT2, bool SEG, int TT, bool MASK, int NT3_, bool WIDE) {
  if (NT < 1 || NT2 < 1 || (NT2 != NT && NT2 != NT - 1) || (TT != 1 && TT != 2)) return false;
  if (WIDE) return NT <= AQ_LA_NT_WIDE && NT2 == NT && TT == 1 && !SEG && NT3_ < 0;
  if (MASK && TT != 1) return false;   // 16 per-trait Gram blocks per trait tile in LDS: one tile per workgroup
  if (NT3_ < 0) return NT <= AQ_LA_NT_UNSPLIT || (NT <= AQ_LA_NT_SPLIT && TT == 1 && !SEG);
  // residual tiles on the recurrence wave of a MASK instance: tried (NT / NT / 3, chained), hung on the GPU; not built
  if (MASK || NT < AQ_LA_NT_REC || NT > AQ_LA_NT_UNSPLIT || NT2 != aq_la_rec_nt2(NT, NT3_)) return false;
  return TT == 1 ? (NT3_ == 3 || NT3_ == 6 || NT3_ == 9) : (NT3_ == 9 && AQ_LA_TT2_REC9);
}

// Generic kernel aq_trait_wave_kernel<NE, WPT>: NE samples per lane, WPT waves per trait; one wave holds at most 32 per lane.
constexpr int AQ_TW_NE[] = {4, 8, 16, 32, 40}, AQ_TW_WPT[] = {1, 2, 4};
constexpr bool aq_tw_built(int NE, int WPT) {
  bool ne = false, wpt = false;
  for (int v : AQ_TW_NE) ne = ne || v == NE;
  for (int v : AQ_TW_WPT) wpt = wpt || v == WPT;
  return ne && wpt && (NE <= 32 || WPT > 1);
}
constexpr int aq_tw_ne_max(int WPT) {   // the largest NE built for this WPT (the lists ascend)
  int m = 0;
  for (int v : AQ_TW_NE) if (aq_tw_built(v, WPT)) m = v;
  return m;
}

// Masked kernel aq_core_sweep_mis_kernel<NT>: NT residual tiles per wave.
constexpr int AQ_MIS_NT[] = {1, 2, 4, 8, 16};
constexpr bool aq_mis_built(int NT) {
  for (int v : AQ_MIS_NT) if (v == NT) return true;
  return false;
}
