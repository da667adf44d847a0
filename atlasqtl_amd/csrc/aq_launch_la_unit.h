// aq_launch_la_unit.h -- the body of every aq_launch_la*.hip unit: aq_la_unit<TT, MASK, WIDE> walks the box of template
// parameters at compile time, instantiates the kernel wherever aq_la_built (aq_plan_const.h) holds and launches the instance
// whose parameters equal the request.  The one place where the look-ahead kernel is launched.
#pragma once
#include "aq_launch_la.h"
#include "aq_core_sweep_la.h"

// the box: NT = 1 ... AQ_LA_NT_SPLIT (or _WIDE) x NT2 in {NT, NT - 1} x SEG x NT3_ in {-1, AQ_LA_REC_FORMS}; I numbers its cells
constexpr int AQ_LA_NFORM = 1 + (int)(sizeof AQ_LA_REC_FORMS / sizeof *AQ_LA_REC_FORMS);
constexpr int AQ_LA_BOX = (AQ_LA_NT_SPLIT > AQ_LA_NT_WIDE ? AQ_LA_NT_SPLIT : AQ_LA_NT_WIDE) * 4 * AQ_LA_NFORM;

template <int TT, bool MASK, bool WIDE>
static int aq_la_unit(const AqLaRequest &rq, const AqLaRun &run) {
  if (rq.TT != TT || rq.mask != MASK || rq.wide != WIDE) return -1;
  return aq_first_arm<AQ_LA_BOX>([&](auto cell) -> int {
    constexpr int I = decltype(cell)::value;
    constexpr int NT = I / (4 * AQ_LA_NFORM) + 1, NT2 = NT - I / (2 * AQ_LA_NFORM) % 2;
    constexpr bool SEG = I / AQ_LA_NFORM % 2 != 0;
    constexpr int NT3_ = I % AQ_LA_NFORM ? AQ_LA_REC_FORMS[I % AQ_LA_NFORM - 1] : -1;
    if constexpr (aq_la_built(NT, NT2, SEG, TT, MASK, NT3_, WIDE)) {
      constexpr int NT3 = aq_la_rec_tiles(NT, NT2, TT, NT3_);
      if (rq.NT != NT || rq.NT2 != NT2 || rq.seg != SEG || rq.rec != NT3) return -1;
      if (run.dry) { run.dry->nt = NT; run.dry->nt2 = NT2; run.dry->seg = SEG; run.dry->tt = TT; run.dry->mask = MASK; run.dry->nt3 = NT3; run.dry->wide = WIDE; }
      else hipLaunchKernelGGL((aq_core_sweep_la_kernel<NT, NT2, SEG, TT, MASK, NT3_, WIDE>), dim3(run.grid), dim3(512), 0, run.st, *run.a);
      return 0;
    }
    return -1;
  });
}
