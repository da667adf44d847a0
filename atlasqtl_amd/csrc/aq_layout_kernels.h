// aq_layout_kernels.h -- the two conversions between R's column-major matrices and the trait-tiled device layout.
// Non-template kernels: included by aq_vb_query.hip only, which puts them behind aq_tile_from_colmajor and aq_colmajor_copy
// (aq_internal.h).
#pragma once
#include <hip/hip_runtime.h>

// (rows x q) R column-major  ->  [ntile][rows_pad][16] trait-tiled; zero padded.
// grid (ceil(rows_pad/64), ntile), 256 threads.  nan_to_zero: Y with NA -> 0 (R/atlasqtl_global_local_core.R:22)
__global__ void aq_k_tile_from_colmajor(const double *__restrict__ src, double *__restrict__ dst, int rows, int q,
                                        int rows_pad, int nan_to_zero) {
  __shared__ double buf[16][65];
  int tile = blockIdx.y;
  int r0 = blockIdx.x * 64;
  for (int e = threadIdx.x; e < 16 * 64; e += 256) {
    int k = e >> 6, rr = e & 63;
    int kk = tile * 16 + k, r = r0 + rr;
    double v = 0.0;
    if (kk < q && r < rows) {
      v = src[(size_t)r + (size_t)rows * kk];
      if (nan_to_zero && v != v) v = 0.0;
    }
    buf[k][rr] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 16 * 64; e += 256) {
    int rr = e >> 4, k = e & 15;
    int r = r0 + rr;
    if (r < rows_pad) dst[((size_t)tile * rows_pad + r) * 16 + k] = buf[k][rr];
  }
}

// trait-tiled -> column-major (rows x q); mul != NULL gives src*mul (beta_vb = gam_vb * mu_beta_vb, R/update_vb.R:17)
__global__ void aq_k_colmajor_from_tile(const double *__restrict__ src, const double *__restrict__ mul,
                                        double *__restrict__ dst, int rows, int q, int rows_pad) {
  __shared__ double buf[16][65];
  int tile = blockIdx.y;
  int r0 = blockIdx.x * 64;
  for (int e = threadIdx.x; e < 16 * 64; e += 256) {
    int rr = e >> 4, k = e & 15;
    int r = r0 + rr;
    double v = 0.0;
    if (r < rows_pad) {
      size_t off = ((size_t)tile * rows_pad + r) * 16 + k;
      v = src[off];
      if (mul) v *= mul[off];
    }
    buf[k][rr] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 16 * 64; e += 256) {
    int k = e >> 6, rr = e & 63;
    int kk = tile * 16 + k, r = r0 + rr;
    if (kk < q && r < rows) dst[(size_t)r + (size_t)rows * kk] = buf[k][rr];
  }
}
