// aq_ytrans_plan.h -- the launch plan of the rank-based inverse normal transform of Y (aq_rank_int, aq_prepare_data_opt;
// kernels in aq_ytrans_kernels.h): which of the two kernels sorts a column, the padded key count, the LDS it asks for, how
// many traits share one launch and the scratch they need, from n, q, the free device memory and the AQ_YT_PATH override.  A
// pure function in the manner of aq_grm_plan.h: integer arithmetic only, no HIP call, no getenv.  The entries run it before
// they allocate the scratch; aq_ytrans_plan_query exposes it on the C ABI without a device.
//
// One workgroup sorts the order-preserving 64-bit keys of one trait, padded to a power of two with the key of a missing
// value.  LDS path: the keys of the column live in LDS (n_pad <= AQ_YT_LDS_KEYS = 16 384 keys = 128 KiB of the 160 KiB of a CU,
// one workgroup per CU).  Global path: the keys of `traits_per_batch` traits live in device memory, n_pad each; chunks of
// min(n_pad, AQ_YT_LDS_KEYS) keys are sorted and merged in LDS, the wider strides of the network run on device memory.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/atlasqtl_hip.h"
#include "aq_plan_const.h"   // AQ_N_MAX

#define AQ_YT_LDS_KEYS 16384     // keys of one column that LDS holds: 128 KiB
#define AQ_YT_LDS_LIMIT 163840   // LDS of a CU (gfx950): 160 KiB
#define AQ_YT_MAX_BATCH 1024     // traits per launch of the global path: four workgroups per CU of work, 1 GiB at n_pad = 2^17
#define AQ_YT_FORCE_LDS 1        // AQ_YT_PATH=lds
#define AQ_YT_FORCE_GLOBAL 2     // AQ_YT_PATH=global

static inline int aq_yt_next_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

// force: 0, AQ_YT_FORCE_LDS or AQ_YT_FORCE_GLOBAL; a forced path that the column does not fit is not taken
static inline int aq_ytrans_make_plan(int n, int q, long long free_bytes, int force, const char *who, aq_ytrans_plan *pl, std::string *err) {
  if (n < 2 || q < 1 || free_bytes < 0) {
    if (err) *err = std::string(who) + ": n >= 2, q >= 1 and free_bytes >= 0 required";
    return AQ_ERR_ARG;
  }
  if (force < 0 || force > AQ_YT_FORCE_GLOBAL) {
    if (err) *err = std::string(who) + ": AQ_YT_PATH must be lds or global";
    return AQ_ERR_ARG;
  }
  if (n > AQ_N_MAX) {
    if (err)
      *err = std::string(who) + ": n = " + std::to_string(n) + " exceeds the largest supported sample count, n <= " + std::to_string(AQ_N_MAX) +
             " (AQ_N_MAX)";
    return AQ_ERR_UNSUPPORTED;
  }
  const int n_pad = aq_yt_next_pow2(n);
  const bool global = n_pad > AQ_YT_LDS_KEYS || force == AQ_YT_FORCE_GLOBAL;
  const long long col_bytes = (long long)n_pad * (long long)sizeof(uint64_t);
  long long batch = q;
  if (global) {
    if (batch > AQ_YT_MAX_BATCH) batch = AQ_YT_MAX_BATCH;
    if (batch > free_bytes / col_bytes) batch = free_bytes / col_bytes;
    if (batch < 1) {
      if (err)
        *err = std::string(who) + ": the keys of one column need " + std::to_string(col_bytes) + " bytes of device memory, " +
               std::to_string(free_bytes) + " are free";
      return AQ_ERR_UNSUPPORTED;
    }
  }
  pl->path = global ? 1 : 0;
  pl->n_pad = n_pad;
  pl->lds_bytes = (int32_t)((n_pad < AQ_YT_LDS_KEYS ? n_pad : AQ_YT_LDS_KEYS) * (long long)sizeof(uint64_t));
  pl->traits_per_batch = (int32_t)batch;
  pl->scratch_bytes = global ? batch * col_bytes : 0;
  return AQ_OK;
}
