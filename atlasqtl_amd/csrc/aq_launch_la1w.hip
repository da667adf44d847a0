// aq_launch_la1w.hip -- instances of the look-ahead sweep kernel for the wide sample split (WIDE: 9 <= C <= AQ_LA_CMAX parts,
// complete Y, one trait tile per workgroup, NT2 == NT, unchained; see aq_launch_la.h).
#include "aq_launch_la.h"
#include "aq_core_sweep_la.h"

int aq_la_launch_wide(int NT, unsigned grid, hipStream_t st, const AqCoreArgs &a) {
#define AQ_LW(NT_) \
  if (NT == NT_) { hipLaunchKernelGGL((aq_core_sweep_la_kernel<NT_, NT_, false, 1, false, -1, true>), dim3(grid), dim3(512), 0, st, a); return 0; }
  AQ_LW(1) AQ_LW(2) AQ_LW(3) AQ_LW(4) AQ_LW(5) AQ_LW(6) AQ_LW(7) AQ_LW(8) AQ_LW(9)
  AQ_LW(10) AQ_LW(11) AQ_LW(12) AQ_LW(13) AQ_LW(14) AQ_LW(15) AQ_LW(16) AQ_LW(17) AQ_LW(18)
#undef AQ_LW
  return -1;
}
