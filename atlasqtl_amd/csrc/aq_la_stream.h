// aq_la_stream.h -- the look-ahead sweep kernel's operand stream and small device primitives: the hand-issued loads with their
// vmcnt waits, the LDS-DMA transfer, the residual's agent-scope access, the DPP row sum, the compile-time loop.  The request
// order of the deep prefetch lives in aq_la_req.h (plain C++).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>
#include "aq_la_req.h"

typedef double aq_v2 __attribute__((ext_vector_type(2)));

// Sum over the 16 lanes of a DPP row (lanes 16 k .. 16 k + 15), result in every lane: quad butterflies, then row rotations by
// 4 and 8 (every quad holds its own sum by then).  Eight v_mov_b32 DPP + four v_add_f64 with register latency, where
// __shfl_xor costs eight ds_bpermute_b32 round trips through the LDS pipeline.
__device__ __forceinline__ double aq_row16_sum(double v) {
  auto step = [&](auto ctrl) __attribute__((always_inline)) {
    constexpr int C = decltype(ctrl)::value;
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), C, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), C, 0xf, 0xf, false);
    v += __hiloint2double(hi, lo);
  };
  step(std::integral_constant<int, 0xB1>{});    // quad_perm [1,0,3,2]
  step(std::integral_constant<int, 0x4E>{});    // quad_perm [2,3,0,1]
  step(std::integral_constant<int, 0x124>{});   // row_ror:4
  step(std::integral_constant<int, 0x128>{});   // row_ror:8
  return v;
}

// cache policy of the Gram-block stream (49 KB per phase and workgroup, read once per sweep): 2 = nt, non-temporal, so that it
// does not push the X operand panels -- which every workgroup of the XCD re-reads -- out of the L2
#ifndef AQ_GLDS_AUX
#define AQ_GLDS_AUX 2
#endif
// One LDS-DMA transfer (global_load_lds_dwordx4): 64 lanes x 16 B from per-lane global addresses to lds_base + 16 lane, with
// no VGPR destination; completion is counted in vmcnt.  lds_base must be wave-uniform.
__device__ __forceinline__ void aq_glds16(const void *gsrc_lane, void *lds_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc_lane,
                                   (__attribute__((address_space(3))) void *)lds_base, 16, 0, AQ_GLDS_AUX);
}

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>).  The residual tiles live in
// registers only while every index into them is a constant expression.
template <int... Is, class F>
__device__ __forceinline__ void aq_static_for_impl(std::integer_sequence<int, Is...>, F &&f) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void aq_static_for(F &&f) {
  aq_static_for_impl(std::make_integer_sequence<int, N>{}, f);
}

// two 16-byte loads (one operand tile = 2 x 1 KB per wave): lane address = sbase + voff (+ 1024).  The base is wave-uniform
// but computed inside the role split, where the compiler no longer proves it: v_readfirstlane puts it into the SGPR pair the
// saddr form needs (folded away wherever uniformity is known).
#define AQ_LD2(d0, d1, voff, sbase)                                                                            \
  do {                                                                                                          \
    const unsigned long long b_ = (unsigned long long)(sbase);                                                  \
    const unsigned lo_ = __builtin_amdgcn_readfirstlane((unsigned)b_);                                          \
    const unsigned hi_ = __builtin_amdgcn_readfirstlane((unsigned)(b_ >> 32));                                  \
    const unsigned long long u_ = ((unsigned long long)hi_ << 32) | lo_;                                        \
    asm volatile("global_load_dwordx4 %0, %2, %3\n\tglobal_load_dwordx4 %1, %2, %3 offset:1024"                \
                 : "=&v"(d0), "=&v"(d1)                                                                         \
                 : "v"(voff), "s"(u_));                                                                         \
  } while (0)
// the same with a compile-time byte offset IMM (and IMM + 1024) in the instruction: one SGPR base serves four tiles
// (IMM in {-4096, -2048, 0, 2048}; the 13-bit signed offset field holds -4096 .. 4095)
#define AQ_LD2I(d0, d1, voff, sbase, IMM)                                                                      \
  do {                                                                                                          \
    const unsigned long long b_ = (unsigned long long)(sbase);                                                  \
    const unsigned lo_ = __builtin_amdgcn_readfirstlane((unsigned)b_);                                          \
    const unsigned hi_ = __builtin_amdgcn_readfirstlane((unsigned)(b_ >> 32));                                  \
    const unsigned long long u_ = ((unsigned long long)hi_ << 32) | lo_;                                        \
    asm volatile("global_load_dwordx4 %0, %2, %3 offset:%4\n\tglobal_load_dwordx4 %1, %2, %3 offset:%5"        \
                 : "=&v"(d0), "=&v"(d1)                                                                         \
                 : "v"(voff), "s"(u_), "i"(IMM), "i"((IMM) + 1024));                                            \
  } while (0)
// one 4-byte load whose value nobody reads (L2 warm-up): lane address = sbase + voff, sbase wave-uniform as above
#define AQ_TOUCH(d, voff, sbase)                                                                               \
  do {                                                                                                          \
    const unsigned long long b_ = (unsigned long long)(sbase);                                                  \
    const unsigned lo_ = __builtin_amdgcn_readfirstlane((unsigned)b_);                                          \
    const unsigned hi_ = __builtin_amdgcn_readfirstlane((unsigned)(b_ >> 32));                                  \
    const unsigned long long u_ = ((unsigned long long)hi_ << 32) | lo_;                                        \
    asm volatile("global_load_dword %0, %1, %2" : "=v"(d) : "v"(voff), "s"(u_));                                \
  } while (0)
// wait until at most N of this wave's vector-memory operations are outstanding; the operands tie the wait to the
// registers it covers so that no use can be scheduled above it
#define AQ_WAIT2(N, d0, d1) asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"(d0), "+v"(d1))
template <int N>
__device__ __forceinline__ void aq_wait2n(aq_v2 &d0, aq_v2 &d1) {   // the same with a count computed at compile time
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(d0), "+v"(d1) : "n"(N));
}

// One word of the residual R.  COH (the chained instances): as an agent-scope relaxed atomic -- global_load / global_store with
// sc1: the load is served past the CU's vector L1, the store is written through to the level every XCD reads -- so that the
// residual passes from one segment's workgroup to the next without a fence (see the hand-over at the end of the kernel).
// Otherwise a plain access.
template <bool COH>
__device__ __forceinline__ double aq_r_load(const double *p) {
  if constexpr (COH) return __hip_atomic_load(const_cast<double *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <bool COH>
__device__ __forceinline__ void aq_r_store(double *p, double v) {
  // (through a global-address-space pointer: where the compiler has lost track of the space it would issue a flat store)
  if constexpr (COH) __hip_atomic_store((__attribute__((address_space(1))) double *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

#ifndef AQ_DEEP_TT1
#define AQ_DEEP_TT1 4   // buffers per operand stream of the one-tile workgroups
#endif
