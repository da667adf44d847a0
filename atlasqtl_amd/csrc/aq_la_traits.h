// aq_la_traits.h -- the constants the look-ahead sweep kernel derives from its seven template parameters, in one place: the
// kernel and every piece of it read them from here.
#pragma once
#include "aq_plan_const.h"   // aq_la_nt3
#include "aq_la_flags.h"     // AQ_FL_NMATRIX

template <int NT_, int NT2_, bool SEG_, int TT_, bool MASK_, int NT3_, bool WIDE_>
struct AqLaTraits {
  static constexpr int NT = NT_, NT2 = NT2_, TT = TT_;
  static constexpr bool SEG = SEG_, MASK = MASK_, WIDE = WIDE_;
  static_assert(!MASK || TT == 1, "the masked form keeps 16 per-trait Gram blocks in LDS: one trait tile per workgroup");
  static_assert(!WIDE || (TT == 1 && !SEG), "the wide sample split: one trait tile per workgroup, never chained");
  static constexpr int NWM = AQ_FL_NMATRIX;              // matrix waves: 0,1,2,4,5,6
  // residual tiles of the recurrence wave (its matrix work follows its chain): aq_la_nt3 unless the instance names its own count
  static constexpr int NT3 = NT3_ >= 0 ? NT3_ : aq_la_nt3(NT, NT2, TT);
  static constexpr int NPS = NWM + (NT3 > 0 ? 1 : 0);    // partial S' slots
  static constexpr int NTR = 16 * TT;                    // traits per workgroup
  static constexpr int ENT = 256 * TT;                   // entries of one SNP block: [snp][trait]
  static constexpr int NG = 4 / TT;                      // 16*TT-lane groups of the recurrence / helper wave
  static constexpr int RPG = 16 / NG;                    // SNP rows per group
  // Complete Y, where the cross-block correction X_b'X_{b-1} delta_{b-1} comes from: with two trait tiles per workgroup the matrix
  // SIMDs are the bound and the helper wave forms the product after each chain (Lcx); with ONE tile per workgroup (the trait
  // shards of a multi-GPU run, small q: the chain is the critical path) it is accumulated INSIDE the chain of block b-1, one
  // column of X_b'X_{b-1} per step as that step's delta appears -- complete the moment that chain ends (CXC).  The chain of
  // block b-1 then needs block b's cross Gram: three buffers, block m in LGx[m % 3], staged a block earlier.
  static constexpr bool CXC = (TT == 1) && !MASK;
  static constexpr int NTT = 3 * (NT + NT2) + NT3;       // residual tiles of a workgroup = 16-sample tiles of a part
};
