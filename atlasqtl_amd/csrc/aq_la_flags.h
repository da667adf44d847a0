// aq_la_flags.h -- the hand-off protocol of the look-ahead sweep kernel's eight waves: the LDS progress counters by name, the
// signal and the waits on them, and the diagnostic builds' wait accounting and timeline marks.
#pragma once
#include <hip/hip_runtime.h>

// Point-to-point progress counters instead of a workgroup barrier per phase: Fl[0..5] = number of SNP blocks whose
// partial S' matrix wave m has written, Fl[6] = blocks the recurrence wave has finished, Fl[7] = blocks the helper
// wave has staged, Fl[8..10] = phases that matrix wave 0..2 has carried past its stagger tile (its SIMD partner 4..6
// starts the phase then), Fl[11] = phases the recurrence wave's own matrix work has finished (init mode: the helper may
// then reuse a beta buffer), Fl[12] = (complete Y) blocks whose cross-block correction the helper wave has put into Lcx, Fl[13] = (MASK) chains that have read their cross blocks, Fl[14] = (sample split) blocks whose
// S' the helper wave has exchanged with the other parts.  Each wave waits only for what it really reads, so the matrix waves -- the critical path --
// never stop at a barrier.  LDS operations of a wave execute in order and the LDS is one pipeline per CU, so
// "data stores; s_waitcnt lgkmcnt(0); counter store" on one side and "counter load ... ; data loads" on the other are
// ordered; the asm memory clobbers keep the compiler from moving accesses across them.
enum AqLaFlag : int {
  AQ_FL_MATRIX = 0,       // + matrix-wave index 0..5 (aq_fl_matrix): SNP blocks whose partial S' that wave has written
  AQ_FL_REC_DONE = 6,     // blocks the recurrence wave has finished (init mode: blocks whose beta the helper wave has put out)
  AQ_FL_STAGED = 7,       // blocks the helper wave has staged
  AQ_FL_STAGGER = 8,      // + matrix wave 0..2 (aq_fl_stagger): phases that wave has carried past its stagger tile
  AQ_FL_REC_TILES = 11,   // phases the recurrence wave's own matrix work has finished
  AQ_FL_CX_READY = 12,    // (complete Y) blocks whose cross-block correction the helper wave has put into Lcx
  AQ_FL_XBLOCK_READ = 13, // (MASK) chains that have read their cross blocks
  AQ_FL_EXCHANGED = 14,   // (sample split) blocks whose S' the helper wave has exchanged with the other parts
  AQ_FL_COUNT = 16        // words of the counter array
};
constexpr int AQ_FL_NMATRIX = 6;   // matrix waves, each with a counter of its own
__device__ __forceinline__ constexpr AqLaFlag aq_fl_matrix(int mw) { return (AqLaFlag)(AQ_FL_MATRIX + mw); }
__device__ __forceinline__ constexpr AqLaFlag aq_fl_stagger(int mw) { return (AqLaFlag)(AQ_FL_STAGGER + mw); }
// wait_s_and_staged reads the counters 0..7 as two 16-byte words and takes the minimum of all but the recurrence wave's own:
// that is "six matrix counters, own counter, helper" by position, in an array aligned to 16 bytes (the workgroup's `__shared__
// AqLaFlagWords Fl`)
struct __attribute__((aligned(16))) AqLaFlagWords { int v[AQ_FL_COUNT]; };
static_assert(AQ_FL_MATRIX == 0 && AQ_FL_NMATRIX == 6 && AQ_FL_REC_DONE == 6 && AQ_FL_STAGED == 7,
              "wait_s_and_staged: words 0..5 the matrix waves, word 6 the recurrence wave's own, word 7 the helper's");
static_assert(alignof(AqLaFlagWords) == 16 && sizeof(AqLaFlagWords) >= 32, "wait_s_and_staged: two aligned 16-byte reads");
static_assert(AQ_FL_STAGGER + 3 == AQ_FL_REC_TILES && AQ_FL_EXCHANGED < AQ_FL_COUNT, "one word per counter");

// (explicit LDS address space: through a generic pointer the volatile accesses become flat loads with a vmcnt(0) drain)
typedef __attribute__((address_space(3))) volatile int aq_lds_vint;
typedef int aq_i4 __attribute__((ext_vector_type(4)));

// One wave's view of the counters.  Flv = the workgroup's counter array, lane / w = this lane and wave, dbg = a.dbg.
struct AqLaFlags {
  aq_lds_vint *Flv;
  int lane, w;
  long long *dbg;
#ifdef AQ_DIAG_TIME
  long long dg_wait = 0, dg_wait_b = 0;   // waits on the matrix / recurrence counters; on the helper's and the stagger counters
  const long long dg_t0 = __builtin_readcyclecounter();
#endif
  __device__ __forceinline__ void signal(AqLaFlag idx, int val) const {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) Flv[idx] = val;
  }
#if defined(AQ_DIAG_TIME) || defined(AQ_DIAG_TL)   // (AQ_DIAG_TL: the timeline marks alone -- a lighter build for instances whose
                                                    // registers the wait counters would push over the edge)
  // timeline of workgroup 0, phases 64 .. 95: slot k of (wave, phase) <- cycle counter (behind the per-wave counters in a.dbg)
  __device__ __forceinline__ void tl_mark(int i, int k) const {
    if (dbg && blockIdx.x == 0 && i >= 64 && i < 96 && lane == 0)
      dbg[(size_t)gridDim.x * 24 + ((size_t)w * 32 + (i - 64)) * 8 + k] = __builtin_readcyclecounter();
  }
#else
  __device__ __forceinline__ void tl_mark(int, int) const {}
#endif
  __device__ __forceinline__ void wait_ge(AqLaFlag idx, int val) {
#ifdef AQ_DIAG_TIME
    const long long t_in = __builtin_readcyclecounter();
#endif
    while (Flv[idx] < val) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
#ifdef AQ_DIAG_TIME
    if (idx >= AQ_FL_STAGED) dg_wait_b += __builtin_readcyclecounter() - t_in;
    else dg_wait += __builtin_readcyclecounter() - t_in;
#endif
  }
  // the recurrence wave's wait at the top of a chain -- all six matrix waves' partial S' and the helper's staging -- as ONE poll of
  // two 16-byte LDS reads instead of seven round trips in a row (0.3 us per SNP block where the chain is the critical path)
  __device__ __forceinline__ void wait_s_and_staged(int val) {
    typedef __attribute__((address_space(3))) volatile aq_i4 aq_lds_vi4;
    aq_lds_vi4 *fp = (aq_lds_vi4 *)Flv;
#ifdef AQ_DIAG_TIME
    const long long t_in = __builtin_readcyclecounter();
#endif
    for (;;) {
      const aq_i4 f0 = fp[0], f1 = fp[1];   // Fl[0..3], Fl[4..7]; Fl[6] is this wave's own counter
      const int lo = min(min(min(f0.x, f0.y), min(f0.z, f0.w)), min(min(f1.x, f1.y), f1.w));
      if (lo >= val) break;
      __builtin_amdgcn_s_sleep(1);
    }
    asm volatile("" ::: "memory");
#ifdef AQ_DIAG_TIME
    dg_wait += __builtin_readcyclecounter() - t_in;
#endif
  }
};
