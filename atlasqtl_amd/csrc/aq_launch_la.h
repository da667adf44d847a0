// aq_launch_la.h -- launch dispatch of the look-ahead sweep kernel (aq_core_sweep_la.h).  The template instances are compiled
// in five translation units so that the library builds in parallel: aq_launch_la1.hip (one trait tile per workgroup),
// aq_launch_la2.hip (two), aq_launch_la1m.hip (MASK: Y with missing values), aq_launch_la1w.hip and aq_launch_la1wm.hip (the
// wide sample split, complete Y and MASK).  Which instances exist is aq_la_built's to say (aq_plan_const.h); each unit
// compiles those of its (TT, MASK, WIDE) and finds the one a request names by the same walk (aq_launch_la_unit.h).
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/atlasqtl_hip.h"
#include "aq_core_sweep.h"

// The compile-time range walk of every dispatch: arm(std::integral_constant<int, I>) for I = 0 ... N - 1 until one answers
// >= 0 (an arm that is not the requested one answers -1); -1 when none does.
template <class Arm, int... I>
int aq_first_arm(Arm &&arm, std::integer_sequence<int, I...>) {
  int rc = -1;
  (void)(((rc = arm(std::integral_constant<int, I>{})) >= 0) || ...);
  return rc;
}
template <int N, class Arm>
int aq_first_arm(Arm &&arm) { return aq_first_arm(arm, std::make_integer_sequence<int, N>{}); }

// A request, in the terms of aq_vb_status: tiles_matrix, tiles_matrix2, tiles_recurrence, tiles_per_group and the three
// instance_flags.  rec is the count the recurrence wave ends up with (aq_la_rec_tiles), whoever names it.
struct AqLaRequest { int NT, NT2, rec, TT; bool seg, mask, wide; };
// A launch on `grid` workgroups of 512 threads -- or, with dry set, none: the template parameters of the instance the request
// resolves to are written there (NT3 as the kernel resolves its NT3_) and no device is touched.
struct AqLaRun { unsigned grid; hipStream_t st; const AqCoreArgs *a; aq_kernel_instance *dry; };

// the units: 0, or -1 when the unit holds no instance for the request
int aq_la_unit_tt1(const AqLaRequest &rq, const AqLaRun &run);
int aq_la_unit_tt2(const AqLaRequest &rq, const AqLaRun &run);
int aq_la_unit_mask(const AqLaRequest &rq, const AqLaRun &run);
int aq_la_unit_wide(const AqLaRequest &rq, const AqLaRun &run);
int aq_la_unit_wide_mask(const AqLaRequest &rq, const AqLaRun &run);

// The one entry point: selects the unit.  Returns 0, or -1 when no instance is compiled for the request.
inline int aq_la_launch(const AqLaRequest &rq, unsigned grid, hipStream_t st, const AqCoreArgs *a, aq_kernel_instance *dry = nullptr) {
  const AqLaRun run{grid, st, a, dry};
  return rq.wide ? (rq.mask ? aq_la_unit_wide_mask(rq, run) : aq_la_unit_wide(rq, run))
         : rq.mask ? aq_la_unit_mask(rq, run)
         : rq.TT == 2 ? aq_la_unit_tt2(rq, run) : aq_la_unit_tt1(rq, run);
}
