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
constexpr int aq_la_nt3(int NT, int NT2, int TT) { return (TT == 2 && NT >= 8) ? (NT2 == NT ? 3 : 6) : 0; }

#define AQ_MIS_MMAX 1024  // most missing samples of one trait the LDS index lists hold (16-bit indices, padded to 16)
