// aq_cov_kernels.h -- covariate adjustment of the device-side preparation: the columns of X and
// of Y are replaced by their least-squares residuals on W = [1, Z] before the existing pipeline standardises / centres them.
// The host hands over Qt, an orthonormal basis of W's columns stored [D][n] (row l = basis vector l, so that the lanes of a
// wave read consecutive samples of one vector: coalesced); Qt[0][i] = 1 / sqrt(n).  Included by aq_prep_cov.hip.
//
// Both kernels are deterministic and do not depend on the column index: one workgroup of 256 threads per column, thread t
// sums samples t, t + 256, ... in that order, the 64 partial sums of a wave go through one shuffle tree and the four waves'
// sums are added in wave order.  Two bit-identical columns of X therefore give bit-identical residuals, which the bitwise
// duplicate detection that follows relies on.
#pragma once
#include "aq_prep_dev.h"     // aq_xval, aq_block_sum

#define AQ_COV_MAX_D 96      // covariates; D = d + 1 basis vectors with the intercept
#define AQ_COV_CHUNK 32      // dot products a thread accumulates at a time
#define AQ_COV_TOL 1e-10     // absorbed column of X / collinear covariate / Cholesky pivot (include/atlasqtl_hip.h)
#define AQ_COV_ROWS 16       // samples of Qt staged in LDS per step of the masked Gram matrix

// sum over the 64 lanes by a butterfly: every lane ends with the same bits (a + b = b + a at every step)
__device__ __forceinline__ double aq_cov_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// c[l] = sum_i Qt[l][i] val(i) for l in [0, D), into LDS; part: 4 x AQ_COV_CHUNK doubles of LDS.  Ends with a barrier.
template <typename F>
__device__ __forceinline__ void aq_cov_dots(const double *__restrict__ Qt, int n, int D, F val, double *c, double *part) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int l0 = 0; l0 < D; l0 += AQ_COV_CHUNK) {
    const int nl = min(AQ_COV_CHUNK, D - l0);
    double acc[AQ_COV_CHUNK];
#pragma unroll
    for (int l = 0; l < AQ_COV_CHUNK; l++) acc[l] = 0.0;
    for (int i = t; i < n; i += 256) {
      const double v = val(i);
      const double *qp = Qt + (size_t)l0 * n + i;
#pragma unroll
      for (int l = 0; l < AQ_COV_CHUNK; l++)
        if (l < nl) {
          acc[l] += *qp * v;
          qp += n;
        }
    }
#pragma unroll
    for (int l = 0; l < AQ_COV_CHUNK; l++) {
      const double s = aq_cov_wave_sum(acc[l]);
      if (lane == 0) part[w * AQ_COV_CHUNK + l] = s;
    }
    __syncthreads();
    if (t < nl) c[l0 + t] = ((part[t] + part[AQ_COV_CHUNK + t]) + part[2 * AQ_COV_CHUNK + t]) + part[3 * AQ_COV_CHUNK + t];
    __syncthreads();
  }
}

// v - sum_l Qt[l][i] c[l], the terms subtracted in the order of l
__device__ __forceinline__ double aq_cov_project_out(const double *__restrict__ Qt, int n, int D, int i, double v, const double *c) {
  for (int l = 0; l < D; l++) v -= Qt[(size_t)l * n + i] * c[l];
  return v;
}

// X: column j <- x_j - Q (Q' x_j), applied twice (re-orthogonalisation: Q' of the result is at rounding level).
//   s0 = sum_i (x_ij - mean_j)^2, s1 = sum_i xr_ij^2, r2[j] = 1 - s1 / s0 (NaN for a constant column)
//   absorbed[j] = the column is not constant and s1 <= AQ_COV_TOL s0: the covariates explain it, what is left is rounding
//                 noise that scale() would blow up to unit variance
// An absorbed or constant column is written as all 0.0, which the pipeline that follows reports constant.  Xr may be X itself
// (T = double): a thread reads x_ij before it writes xr_ij, and nobody else touches that entry.
template <typename T>
__global__ __launch_bounds__(256) void aq_k_cov_residualise(const T *X, int n, int D, const double *__restrict__ Qt, double *Xr,
                                                           uint8_t *__restrict__ absorbed, double *__restrict__ r2) {
  __shared__ double c[AQ_COV_MAX_D + 1];
  __shared__ double part[4 * AQ_COV_CHUNK];
  __shared__ double sh[256];
  __shared__ int ne;
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * n;
  const double x0 = aq_xval(X, base);
  if (t == 0) ne = 0;
  __syncthreads();
  int diff = 0;
  for (int i = t; i < n; i += 256) diff |= (aq_xval(X, base + i) != x0);
  if (diff) ne = 1;
  aq_cov_dots(Qt, n, D, [&](int i) { return aq_xval(X, base + i); }, c, part);
  const bool is_cst = (ne == 0);
  const double mean = c[0] * Qt[0];          // Qt[0][i] = 1 / sqrt(n): c[0] / sqrt(n) = sum / n
  double s0 = 0.0;
  for (int i = t; i < n; i += 256) {
    const double v = aq_xval(X, base + i);
    const double dv = v - mean;
    s0 += dv * dv;
    Xr[base + i] = aq_cov_project_out(Qt, n, D, i, v, c);
  }
  s0 = aq_block_sum(s0, sh);
  aq_cov_dots(Qt, n, D, [&](int i) { return Xr[base + i]; }, c, part);
  double s1 = 0.0;
  for (int i = t; i < n; i += 256) {
    const double v = aq_cov_project_out(Qt, n, D, i, Xr[base + i], c);
    s1 += v * v;
    Xr[base + i] = v;
  }
  s1 = aq_block_sum(s1, sh);
  const bool gone = !is_cst && s1 <= AQ_COV_TOL * s0;
  if (is_cst || gone)
    for (int i = t; i < n; i += 256) Xr[base + i] = 0.0;
  if (t == 0) {
    absorbed[blockIdx.x] = gone ? 1 : 0;
    r2[blockIdx.x] = is_cst ? __longlong_as_double(0x7ff8000000000000ll) : 1.0 - s1 / s0;
  }
}

__device__ __forceinline__ int aq_cov_tri(int i, int j) { return i * (i + 1) / 2 + j; }   // lower triangle, j <= i

// L L' x = b in place (b -> x), L the lower triangle in LDS; all 256 threads call it, D <= 97 of them work.  z: D doubles.
__device__ __forceinline__ void aq_cov_chol_solve(const double *L, int D, double *b, double *z) {
  const int t = threadIdx.x;
  for (int j = 0; j < D; j++) {
    if (t == j) z[j] = b[j] / L[aq_cov_tri(j, j)];
    __syncthreads();
    if (t > j && t < D) b[t] -= L[aq_cov_tri(t, j)] * z[j];
    __syncthreads();
  }
  for (int j = D - 1; j >= 0; j--) {
    if (t == j) b[j] = z[j] / L[aq_cov_tri(j, j)];
    __syncthreads();
    if (t < j) z[t] -= L[aq_cov_tri(j, t)] * b[j];
    __syncthreads();
  }
}

// Y: one workgroup per trait k with observed rows O_k (NaN = missing, stays NaN):
//   y_k[O_k] <- y_k[O_k] - Q[O_k] b,  b the least-squares solution on those rows: G = Q[O_k]' Q[O_k] (masked Gram matrix,
//   lower triangle in LDS, every entry summed over the samples in order), Cholesky, solve; then once more on the residual
//   (refinement).  G is well conditioned because Q is orthonormal over all rows.  With the intercept in Q this centres the
//   column as well.  nobs[k] = |O_k|; flag[k] = 0 done, 1 |O_k| <= D, 2 a Cholesky pivot <= AQ_COV_TOL (nothing written then).
// Dynamic LDS: D (D + 1) / 2 + AQ_COV_ROWS D + 2 D + 4 AQ_COV_CHUNK + 256 doubles (aq_cov_y_lds_bytes), 54 KB at D = 97.
static inline size_t aq_cov_y_lds_bytes(int D) {
  return ((size_t)D * (D + 1) / 2 + (size_t)AQ_COV_ROWS * D + 2 * (size_t)D + 4 * AQ_COV_CHUNK + 256) * sizeof(double);
}

__global__ __launch_bounds__(256) void aq_k_cov_residualise_y(const double *__restrict__ Y, int n, int D, const double *__restrict__ Qt,
                                                             double *Yc, int *__restrict__ nobs, int *__restrict__ flag) {
  extern __shared__ double lds[];
  const int ntri = D * (D + 1) / 2;
  double *G = lds;                          // ntri
  double *Qs = G + ntri;                    // D x AQ_COV_ROWS: Qs[l][r], 0.0 where the row is missing
  double *b = Qs + AQ_COV_ROWS * D;         // D
  double *z = b + D;                        // D
  double *part = z + D;                     // 4 x AQ_COV_CHUNK
  double *sh = part + 4 * AQ_COV_CHUNK;     // 256
  const int t = threadIdx.x, k = blockIdx.x;
  const size_t base = (size_t)k * n;
  double cnt = 0.0;
  for (int i = t; i < n; i += 256) {
    const double v = Y[base + i];
    cnt += (v == v) ? 1.0 : 0.0;
  }
  const int n_obs = (int)aq_block_sum(cnt, sh);
  if (t == 0) nobs[k] = n_obs;
  if (n_obs <= D) {
    if (t == 0) flag[k] = 1;
    return;
  }
  // masked Gram matrix: AQ_COV_ROWS samples at a time through LDS, entry e = (a, b) of the triangle by thread e mod 256
  for (int e = t; e < ntri; e += 256) G[e] = 0.0;
  for (int i0 = 0; i0 < n; i0 += AQ_COV_ROWS) {
    __syncthreads();
    for (int idx = t; idx < D * AQ_COV_ROWS; idx += 256) {
      const int l = idx / AQ_COV_ROWS, i = i0 + idx % AQ_COV_ROWS;
      double v = 0.0;
      if (i < n) {
        const double y = Y[base + i];
        if (y == y) v = Qt[(size_t)l * n + i];
      }
      Qs[idx] = v;
    }
    __syncthreads();
    for (int e = t; e < ntri; e += 256) {
      int a = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
      while (a * (a + 1) / 2 > e) a--;
      while ((a + 1) * (a + 2) / 2 <= e) a++;
      const int bcol = e - a * (a + 1) / 2;
      const double *qa = Qs + a * AQ_COV_ROWS, *qb = Qs + bcol * AQ_COV_ROWS;
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < AQ_COV_ROWS; r++) s += qa[r] * qb[r];
      G[e] += s;
    }
  }
  __syncthreads();
  // Cholesky in place, column by column: thread t takes row j + t of column j
  for (int j = 0; j < D; j++) {
    const int i = j + t;
    double s = 0.0;
    if (i < D) {
      s = G[aq_cov_tri(i, j)];
      for (int m = 0; m < j; m++) s -= G[aq_cov_tri(i, m)] * G[aq_cov_tri(j, m)];
      G[aq_cov_tri(i, j)] = s;
    }
    __syncthreads();
    const double piv = G[aq_cov_tri(j, j)];
    __syncthreads();
    if (!(piv > AQ_COV_TOL)) {
      if (t == 0) flag[k] = 2;
      return;
    }
    const double ljj = sqrt(piv);
    if (i < D) G[aq_cov_tri(i, j)] = (t == 0) ? ljj : s / ljj;
    __syncthreads();
  }
  // solve, residual; then the same on the residual
  aq_cov_dots(Qt, n, D, [&](int i) { const double y = Y[base + i]; return y == y ? y : 0.0; }, b, part);
  aq_cov_chol_solve(G, D, b, z);
  for (int i = t; i < n; i += 256) {
    const double y = Y[base + i];
    Yc[base + i] = y == y ? aq_cov_project_out(Qt, n, D, i, y, b) : y;
  }
  __syncthreads();
  aq_cov_dots(Qt, n, D, [&](int i) { const double y = Y[base + i]; return y == y ? Yc[base + i] : 0.0; }, b, part);
  aq_cov_chol_solve(G, D, b, z);
  for (int i = t; i < n; i += 256) {
    const double y = Y[base + i];
    if (y == y) Yc[base + i] = aq_cov_project_out(Qt, n, D, i, Yc[base + i], b);
  }
  if (t == 0) flag[k] = 0;
}
