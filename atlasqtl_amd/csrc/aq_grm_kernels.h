// aq_grm_kernels.h -- the genetic relationship matrix of the device-side preparation:
// K = Xs Xs' / p1 over all p1 columns of the compact standardised X, n x n, on the f64 matrix pipe.  Included by
// aq_prep_grm.hip; the launch plan is aq_grm_plan.h.  Every kernel is a plain grid: no workgroup waits for another one,
// nothing spins, and no floating-point atomic is used, so two calls on one handle give the same bits.
//
// Xs is [p1][n], every column contiguous.  K[a, b] = sum_j Xs[a, j] Xs[b, j] / p1.
//
// aq_k_grm_partial<T, A16>, grid (n_tiles, splits), 256 threads; A16 = n is even, chosen by the host.  Workgroup (t, s) owns
// the T x T tile (ti, tj), ti >= tj, of the lower triangle -- samples a0 = T ti ... of the A operand against samples b0 = T tj ... of the B operand -- and the
// predictors [s cps KC, (s + 1) cps KC) of split s.  Predictors go through LDS AQ_GRM_KC at a time as two panels
// P[predictor][sample], read from global memory with every lane taking 16 consecutive bytes of one column in one
// global_load_dwordx4 (A16; two 8-byte loads when n is odd and the columns are not 16-byte aligned: a template argument, since
// a run-time choice inside the loop is folded into the 8-byte form) and T / 2 lanes a run of 8 T bytes; a diagonal tile stages one panel and reads
// both operands from it.  The next chunk is loaded into registers before the current one is multiplied.
// Operands: A and B hold one f64 per lane, lane = 16 k + sample (k = predictor within the step of 4), the 16 samples being
// 16 consecutive doubles of one LDS row; the accumulator has col = lane & 15 (the B sample) and row = (lane >> 4) + 4 reg
// (the A sample): the layout aq_probe_dmode verifies on the device, which aq_prep_grm requires before it launches.
// The four waves tile the output 2 x 2; a wave holds (T / 32)^2 accumulators and per step of 4 predictors issues T / 32
// LDS reads of A and of B for (T / 32)^2 v_mfma_f64_16x16x4_f64.
// LDS rows are T + 16 doubles: ds_read_b64 banks by (byte address / 4) mod 64 within each half wave, a half wave reads 16
// consecutive doubles (32 banks) of rows k and k + 1, and (T + 16) mod 32 = 16 doubles puts the second row on the other 32
// banks.  The row length is even, so a lane's 16-byte store is aligned.
// The partial tile goes to scratch[(t splits + s) T T + r T + c] (r the A sample, c the B sample): 16 lanes write 128
// consecutive bytes.
//
// aq_k_grm_reduce, grid (n_tiles, (T / 16)^2), 256 threads: one 16 x 16 block of a tile.  Adds the partials in the order
// s = 0, 1, ..., divides by p1 and writes K[a0 + r, b0 + c] and its mirror K[b0 + c, a0 + r] from the same register, the one
// through an LDS transpose so that both stores run along a column of K.  Of a diagonal tile only r >= c is used.
#pragma once
#include "aq_grm_plan.h"

typedef double aq_grm_d4 __attribute__((ext_vector_type(4)));

template <int T>
struct AqGrmShape {
  static constexpr int STR = T + 16;                 // doubles per predictor row in LDS
  static constexpr int WT = T / 2;                   // samples per wave and operand
  static constexpr int NI = WT / 16;                 // 16-sample tiles per wave and operand
  static constexpr int NV = (T / 2) * AQ_GRM_KC / 256;   // 16-byte vectors per thread and panel
};

// predictors [j0, j0 + AQ_GRM_KC) x samples [s0, s0 + T) of Xs -> v; 0.0 for a predictor >= j_end and for a sample >= n
// A16: n is even, so every pair starts at a multiple of 16 bytes and ends inside its column: one 16-byte load
template <int T, bool A16>
__device__ __forceinline__ void aq_grm_load(const double *__restrict__ Xs, int n, long long j0, long long j_end, int s0,
                                            double2 (&v)[AqGrmShape<T>::NV]) {
#pragma unroll
  for (int u = 0; u < AqGrmShape<T>::NV; u++) {
    const int idx = threadIdx.x + 256 * u;
    const long long j = j0 + idx / (T / 2);
    const int s = s0 + 2 * (idx % (T / 2));
    double2 x = make_double2(0.0, 0.0);
    if (j < j_end && s < n) {
      const double *src = Xs + (size_t)j * (size_t)n + (size_t)s;
      if (A16) {
        x = *reinterpret_cast<const double2 *>(src);
      } else {
        x.x = src[0];
        if (s + 1 < n) x.y = src[1];
      }
    }
    v[u] = x;
  }
}

template <int T>
__device__ __forceinline__ void aq_grm_store(const double2 (&v)[AqGrmShape<T>::NV], double *P) {
#pragma unroll
  for (int u = 0; u < AqGrmShape<T>::NV; u++) {
    const int idx = threadIdx.x + 256 * u;
    *reinterpret_cast<double2 *>(P + (idx / (T / 2)) * AqGrmShape<T>::STR + 2 * (idx % (T / 2))) = v[u];
  }
}

template <int T, bool A16>
__global__ __launch_bounds__(256) void aq_k_grm_partial(const double *__restrict__ Xs, int n, int p1, int splits, int cps,
                                                       double *__restrict__ scratch) {
  typedef AqGrmShape<T> SH;
  __shared__ double PA[AQ_GRM_KC * SH::STR];
  __shared__ double PB[AQ_GRM_KC * SH::STR];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, l = lane & 15;
  const int wr = w >> 1, wc = w & 1;
  int ti, tj;
  aq_grm_tile_rc((int)blockIdx.x, &ti, &tj);
  const bool diag = ti == tj;
  const int a0 = T * ti, b0 = T * tj;
  const long long j_begin = (long long)blockIdx.y * cps * AQ_GRM_KC;
  const long long j_end = min((long long)p1, j_begin + (long long)cps * AQ_GRM_KC);
  const bool idle = diag && wc > wr;             // the wave above the diagonal of a diagonal tile: its part is never read
  aq_grm_d4 acc[SH::NI][SH::NI];
#pragma unroll
  for (int i = 0; i < SH::NI; i++)
#pragma unroll
    for (int jj = 0; jj < SH::NI; jj++) acc[i][jj] = aq_grm_d4{0.0, 0.0, 0.0, 0.0};
  const double *pa = PA + g * SH::STR + wr * SH::WT + l;
  const double *pb = (diag ? PA : PB) + g * SH::STR + wc * SH::WT + l;
  double2 va[SH::NV], vb[SH::NV];
  if (j_begin < j_end) {
    aq_grm_load<T, A16>(Xs, n, j_begin, j_end, a0, va);
    if (!diag) aq_grm_load<T, A16>(Xs, n, j_begin, j_end, b0, vb);
  }
  for (long long j0 = j_begin; j0 < j_end; j0 += AQ_GRM_KC) {
    __syncthreads();                             // the panels of the previous chunk have been read
    aq_grm_store<T>(va, PA);
    if (!diag) aq_grm_store<T>(vb, PB);
    __syncthreads();
    if (j0 + AQ_GRM_KC < j_end) {
      aq_grm_load<T, A16>(Xs, n, j0 + AQ_GRM_KC, j_end, a0, va);
      if (!diag) aq_grm_load<T, A16>(Xs, n, j0 + AQ_GRM_KC, j_end, b0, vb);
    }
    if (!idle) {
#pragma unroll
      for (int kk = 0; kk < AQ_GRM_KC; kk += 4) {
        double a[SH::NI], b[SH::NI];
#pragma unroll
        for (int i = 0; i < SH::NI; i++) {
          a[i] = pa[kk * SH::STR + 16 * i];
          b[i] = pb[kk * SH::STR + 16 * i];
        }
#pragma unroll
        for (int i = 0; i < SH::NI; i++)
#pragma unroll
          for (int jj = 0; jj < SH::NI; jj++) acc[i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[jj], acc[i][jj], 0, 0, 0);
      }
    }
  }
  double *out = scratch + ((size_t)blockIdx.x * splits + blockIdx.y) * (size_t)(T * T);
#pragma unroll
  for (int i = 0; i < SH::NI; i++)
#pragma unroll
    for (int jj = 0; jj < SH::NI; jj++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int r = wr * SH::WT + 16 * i + g + 4 * reg, c = wc * SH::WT + 16 * jj + l;
        out[r * T + c] = acc[i][jj][reg];
      }
}

__global__ __launch_bounds__(256) void aq_k_grm_reduce(const double *__restrict__ scratch, int T, int n, int p1, int splits,
                                                      double *__restrict__ K) {
  __shared__ double sh[16][17];
  const int x = threadIdx.x & 15, y = threadIdx.x >> 4;
  const int nb = T / 16, rb = 16 * ((int)blockIdx.y / nb), cb = 16 * ((int)blockIdx.y % nb);
  int ti, tj;
  aq_grm_tile_rc((int)blockIdx.x, &ti, &tj);
  const bool diag = ti == tj;
  if (diag && rb + 15 < cb) return;              // a block above the diagonal: written as the mirror of the one below
  const int a0 = T * ti, b0 = T * tj;
  const size_t tt = (size_t)T * T;
  const double *src = scratch + (size_t)blockIdx.x * splits * tt + (size_t)(rb + y) * T + (cb + x);
  double v = 0.0;
  for (int s = 0; s < splits; s++) v += src[(size_t)s * tt];
  v /= (double)p1;
  sh[y][x] = v;
  {                                              // the mirror K[b0 + c, a0 + r]: x runs along the column a0 + r of K
    const int r = rb + y, c = cb + x;
    if (a0 + r < n && b0 + c < n && (!diag || r >= c)) K[(size_t)(a0 + r) * n + (size_t)(b0 + c)] = v;
  }
  __syncthreads();
  {                                              // K[a0 + r, b0 + c]: x runs along the column b0 + c of K
    const int r = rb + x, c = cb + y;
    if (a0 + r < n && b0 + c < n && (!diag || r >= c)) K[(size_t)(b0 + c) * n + (size_t)(a0 + r)] = sh[x][y];
  }
}
