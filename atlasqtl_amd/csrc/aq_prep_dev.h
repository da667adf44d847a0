// aq_prep_dev.h -- the two device helpers that the kernels of the prepare side share, and nothing else: the kernels of
// aq_prepare.hip, aq_cov_kernels.h and aq_pcs_kernels.h.  Every file that uses one includes this header, so none depends on
// what was included before it.  It names no HIP header of its own: tools/cov_kernels_cpu.cpp includes it on the CPU, after its
// own threadIdx, __syncthreads and qualifier macros.
#pragma once
#include <stddef.h>

template <typename T>
__device__ __forceinline__ double aq_xval(const T *X, size_t i) { return (double)X[i]; }

// block-wide sum in a fixed order (tree over 256 threads): deterministic, identical for identical columns
__device__ __forceinline__ double aq_block_sum(double v, double *sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
