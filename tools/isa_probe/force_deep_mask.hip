// tools/isa_probe/force_deep_mask.hip -- ISA study only, never linked into the library, never launched.
// Regenerates the build that faulted in round 2: the four-buffer operand prefetch (DEEP, DB = 4) in the 256-VGPR MASK instance
// <14, 14, false, 1, true> (and its neighbours), which the shipped header denies.  Compile to assembly and run
// tools/check_isa_operands.py over it:
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -DAQ_FORCE_DEEP_DB=4 --cuda-device-only -S -I atlasqtl_amd/csrc \
//         -o /tmp/force_deep_mask.s tools/isa_probe/force_deep_mask.hip
#include "aq_core_sweep_la.h"   // the kernel; it includes the aq_la_*.h headers beside it (stream, counters, derived constants)
template __global__ void aq_core_sweep_la_kernel<14, 14, false, 1, true>(const AqCoreArgs);
template __global__ void aq_core_sweep_la_kernel<14, 13, false, 1, true>(const AqCoreArgs);
template __global__ void aq_core_sweep_la_kernel<12, 12, false, 1, true>(const AqCoreArgs);
template __global__ void aq_core_sweep_la_kernel<11, 10, false, 1, true>(const AqCoreArgs);
