// aq_pcs_kernels.h -- one application of the relationship operator to a block of vectors:
// Z = Xs (Xs' Q) / p1, n x L, without the n x n matrix K = Xs Xs' / p1 itself -- what subspace iteration for the leading
// eigenvectors of K needs.  Two tall-skinny products on the f64 matrix pipe.  Included by aq_prep_grm.hip after
// aq_grm_kernels.h (aq_grm_load / aq_grm_store stage the panels of the second product); the launch plan is aq_pcs_plan.h.
// Every kernel is a plain grid: no workgroup waits for another one, nothing spins, and no floating-point atomic is used, so
// two calls on one handle give the same bits.
//
// Xs is [p1][n], every column contiguous.  lp = L padded to 16; NL = lp / 16 = 1 ... 8 is a template argument: the number of
// accumulators a wave holds in registers, and every LDS row length a compile-time constant.
// MFMA operands as in aq_grm_kernels.h: A and B hold one f64 per lane, lane = 16 k + index (k = position within the step of
// 4 of the reduction); the accumulator has col = lane & 15 (the B index) and row = (lane >> 4) + 4 reg (the A index): the
// layout aq_probe_dmode verifies on the device, which aq_prep_grm_apply requires before it launches.
//
// aq_k_pcs_pack_q: Q (n x L, column-major) -> Qt (n_pad x lp, row-major) with 0.0 in the rows >= n and the columns >= L, so
// that the padding of the first product contributes exact zeros and a chunk of Q is one contiguous run.
//
// aq_k_pcs_xtq<NL, A16>, grid n_panels, 256 threads: T = Xs' Q (p1 x lp, row-major, in HBM).  A16 = n is even, chosen by the
// host.  Workgroup b owns the predictors [64 b, 64 b + 64), wave w the 16 of them from 64 b + 16 w, and all lp columns.
// The reduction runs over the samples, AQ_PCS_NC = 32 at a time.  The A operand comes straight from global memory: lane
// (g, m) = (lane >> 4, lane & 15) takes the samples i0 + 2 g + 8 u, + 1 (u = 0 ... 3) of predictor m in one 16-byte load
// each (two 8-byte loads when n is odd and the columns are not 16-byte aligned, as aq_grm_load does), so four lanes read 64
// consecutive bytes of one column; which sample sits at which k of which MFMA is free as long as B agrees.  The B operand is
// the chunk of Qt, staged in LDS as Qs[sample][lp + 8] and shared by the four waves: lane (g, c) reads Qs[2 g + 8 u + h][16 t
// + c] for the half h = 0, 1 of the pair.  ds_read_b64 banks by (byte address / 4) mod 64 within each half wave, a half wave
// reads 16 consecutive doubles of the rows r and r + 2, and 2 (lp + 8) mod 32 = 16 doubles puts the second on the other 32
// banks.  The next chunk of both operands is loaded into registers before the current one is multiplied.  A predictor >= p1
// or a sample >= n is loaded as 0.0; T has 64 n_panels rows, so every row a workgroup owns is written.
//
// aq_k_pcs_xt<NL, A16>, grid (n_tiles, splits), 256 threads: the partial tiles of Xs T.  Workgroup (t, s) owns the samples
// [64 t, 64 t + 64), wave w the 16 of them from 64 t + 16 w, all lp columns and the predictors [s cps KC, (s + 1) cps KC).
// Predictors go through LDS AQ_PCS_KC = 16 at a time: the panel P[predictor][sample] of Xs exactly as the GRM kernel stages
// it (aq_grm_load<64, A16>, rows of 80 doubles), and the same 16 rows of T as Ts[predictor][lp or lp + 16], the row length
// = 16 mod 32 doubles for the same bank argument.  A = T (row = column c of Z), B = Xs (col = sample), so the accumulator has
// the sample along the lanes and the partial tile goes to scratch[((t splits + s) lp + c) 64 + r] (r the sample) with 16
// lanes writing 128 consecutive bytes.  Rows of T past the split's end meet staged zeros of Xs.
//
// aq_k_pcs_reduce, grid (n_tiles, ceil(L / 4)), 256 threads: adds the partials of one (sample, column) in the order
// s = 0, 1, ..., divides by p1 and writes Z[c n + i] for i < n, c < L.
//
// aq_k_pcs_colss, grid p1, 256 threads: the sum of squares of one column in the fixed order of aq_block_sum; the host adds
// the columns in index order and divides by p1: the trace of K without K.
#pragma once
#include "aq_pcs_plan.h"
#include "aq_prep_dev.h"      // aq_block_sum

typedef double aq_pcs_d2 __attribute__((ext_vector_type(2)));

// Q (n x L, column-major) -> Qt (n_pad x lp, row-major, zero-padded)
__global__ __launch_bounds__(256) void aq_k_pcs_pack_q(const double *__restrict__ Q, int n, int L, int n_pad, int lp,
                                                      double *__restrict__ Qt) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;      // i runs fastest: the reads follow a column of Q
  if (idx >= (long long)n_pad * lp) return;
  const int c = (int)(idx / n_pad), i = (int)(idx % n_pad);
  Qt[(size_t)i * lp + c] = (i < n && c < L) ? Q[(size_t)c * n + i] : 0.0;
}

// samples i0 + 2 g + 8 u, + 1 (u = 0 ... 3) of column `col` (nullptr: a predictor >= p1) -> v; 0.0 for a sample >= n
template <bool A16>
__device__ __forceinline__ void aq_pcs_load_a(const double *__restrict__ col, int n, int i0, int g, double2 (&v)[AQ_PCS_NC / 8]) {
#pragma unroll
  for (int u = 0; u < AQ_PCS_NC / 8; u++) {
    const int s = i0 + 2 * g + 8 * u;
    double2 x = make_double2(0.0, 0.0);
    if (col && s < n) {
      if (A16) {
        x = *reinterpret_cast<const double2 *>(col + s);
      } else {
        x.x = col[s];
        if (s + 1 < n) x.y = col[s + 1];
      }
    }
    v[u] = x;
  }
}

template <int NL, bool A16>
__global__ __launch_bounds__(256) void aq_k_pcs_xtq(const double *__restrict__ Xs, int n, int p1, int n_pad,
                                                   const double *__restrict__ Qt, double *__restrict__ T) {
  constexpr int LP = 16 * NL, STRQ = LP + 8, HALF = LP / 2;
  __shared__ double Qs[AQ_PCS_NC * STRQ];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, l = lane & 15;
  const long long jrow = (long long)blockIdx.x * AQ_PCS_PJ + 16 * w;    // the wave's first predictor
  const long long j = jrow + l;                                         // the predictor this lane loads
  const double *col = j < (long long)p1 ? Xs + (size_t)j * (size_t)n : nullptr;
  aq_grm_d4 acc[NL];
#pragma unroll
  for (int t = 0; t < NL; t++) acc[t] = aq_grm_d4{0.0, 0.0, 0.0, 0.0};
  double2 va[AQ_PCS_NC / 8];
  aq_pcs_d2 vq[NL];
  // a chunk of Qt is 32 LP contiguous doubles = 256 NL pairs: thread x takes the pairs x + 256 u, u < NL
  const aq_pcs_d2 *qsrc = reinterpret_cast<const aq_pcs_d2 *>(Qt) + threadIdx.x;
  aq_pcs_load_a<A16>(col, n, 0, g, va);
#pragma unroll
  for (int u = 0; u < NL; u++) vq[u] = qsrc[256 * u];
  for (int i0 = 0; i0 < n_pad; i0 += AQ_PCS_NC) {
    __syncthreads();                             // the chunk before this one has been read
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int idx = threadIdx.x + 256 * u;
      *reinterpret_cast<aq_pcs_d2 *>(Qs + (idx / HALF) * STRQ + 2 * (idx % HALF)) = vq[u];
    }
    __syncthreads();
    double2 a[AQ_PCS_NC / 8];
#pragma unroll
    for (int u = 0; u < AQ_PCS_NC / 8; u++) a[u] = va[u];
    if (i0 + AQ_PCS_NC < n_pad) {
      aq_pcs_load_a<A16>(col, n, i0 + AQ_PCS_NC, g, va);
      const aq_pcs_d2 *qn = qsrc + (size_t)(i0 + AQ_PCS_NC) * (size_t)HALF;
#pragma unroll
      for (int u = 0; u < NL; u++) vq[u] = qn[256 * u];
    }
    const double *qb = Qs + 2 * g * STRQ + l;
#pragma unroll
    for (int u = 0; u < AQ_PCS_NC / 8; u++) {
#pragma unroll
      for (int t = 0; t < NL; t++) {
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u].x, qb[(8 * u) * STRQ + 16 * t], acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u].y, qb[(8 * u + 1) * STRQ + 16 * t], acc[t], 0, 0, 0);
      }
    }
  }
  double *out = T + (size_t)jrow * (size_t)LP;
#pragma unroll
  for (int t = 0; t < NL; t++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) out[(size_t)(g + 4 * reg) * LP + 16 * t + l] = acc[t][reg];
}

template <int NL, bool A16>
__global__ __launch_bounds__(256) void aq_k_pcs_xt(const double *__restrict__ Xs, int n, int p1, int splits, int cps,
                                                  const double *__restrict__ T, double *__restrict__ scratch) {
  typedef AqGrmShape<AQ_PCS_TS> SH;
  constexpr int LP = 16 * NL, STRT = (NL & 1) ? LP : LP + 16, HALF = LP / 2;
  constexpr int NTV = (NL + 1) / 2;              // 16 rows of T are 8 LP pairs: thread x takes the pairs x + 256 u < 8 LP
  __shared__ double P[AQ_PCS_KC * SH::STR];
  __shared__ double Ts[AQ_PCS_KC * STRT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, l = lane & 15;
  const int s0 = AQ_PCS_TS * (int)blockIdx.x;
  const long long j_begin = (long long)blockIdx.y * cps * AQ_PCS_KC;
  const long long j_end = min((long long)p1, j_begin + (long long)cps * AQ_PCS_KC);
  aq_grm_d4 acc[NL];
#pragma unroll
  for (int t = 0; t < NL; t++) acc[t] = aq_grm_d4{0.0, 0.0, 0.0, 0.0};
  double2 vx[SH::NV], vt[NTV];
#pragma unroll
  for (int u = 0; u < NTV; u++) vt[u] = make_double2(0.0, 0.0);
  if (j_begin < j_end) {
    aq_grm_load<AQ_PCS_TS, A16>(Xs, n, j_begin, j_end, s0, vx);
    const double2 *tsrc = reinterpret_cast<const double2 *>(T + (size_t)j_begin * (size_t)LP);
#pragma unroll
    for (int u = 0; u < NTV; u++)
      if ((int)threadIdx.x + 256 * u < 8 * LP) vt[u] = tsrc[threadIdx.x + 256 * u];
  }
  for (long long j0 = j_begin; j0 < j_end; j0 += AQ_PCS_KC) {
    __syncthreads();                             // the panels of the previous chunk have been read
    aq_grm_store<AQ_PCS_TS>(vx, P);
#pragma unroll
    for (int u = 0; u < NTV; u++) {
      const int idx = threadIdx.x + 256 * u;
      if (idx < 8 * LP) *reinterpret_cast<double2 *>(Ts + (idx / HALF) * STRT + 2 * (idx % HALF)) = vt[u];
    }
    __syncthreads();
    if (j0 + AQ_PCS_KC < j_end) {
      aq_grm_load<AQ_PCS_TS, A16>(Xs, n, j0 + AQ_PCS_KC, j_end, s0, vx);
      const double2 *tsrc = reinterpret_cast<const double2 *>(T + (size_t)(j0 + AQ_PCS_KC) * (size_t)LP);
#pragma unroll
      for (int u = 0; u < NTV; u++)
        if ((int)threadIdx.x + 256 * u < 8 * LP) vt[u] = tsrc[threadIdx.x + 256 * u];
    }
    const double *pb = P + g * SH::STR + 16 * w + l;
    const double *pa = Ts + g * STRT + l;
#pragma unroll
    for (int kk = 0; kk < AQ_PCS_KC; kk += 4) {
      const double b = pb[kk * SH::STR];
#pragma unroll
      for (int t = 0; t < NL; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk * STRT + 16 * t], b, acc[t], 0, 0, 0);
    }
  }
  double *out = scratch + ((size_t)blockIdx.x * splits + blockIdx.y) * (size_t)(AQ_PCS_TS * LP);
#pragma unroll
  for (int t = 0; t < NL; t++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) out[(16 * t + g + 4 * reg) * AQ_PCS_TS + 16 * w + l] = acc[t][reg];
}

__global__ __launch_bounds__(256) void aq_k_pcs_reduce(const double *__restrict__ scratch, int n, int p1, int L, int lp, int splits,
                                                      double *__restrict__ Z) {
  const int r = threadIdx.x & 63, c = 4 * (int)blockIdx.y + (threadIdx.x >> 6);
  const int i = AQ_PCS_TS * (int)blockIdx.x + r;
  if (c >= L || i >= n) return;
  const size_t tt = (size_t)AQ_PCS_TS * lp;
  const double *src = scratch + (size_t)blockIdx.x * splits * tt + (size_t)c * AQ_PCS_TS + r;
  double v = 0.0;
  for (int s = 0; s < splits; s++) v += src[(size_t)s * tt];
  Z[(size_t)c * n + i] = v / (double)p1;
}

__global__ __launch_bounds__(256) void aq_k_pcs_colss(const double *__restrict__ Xs, int n, double *__restrict__ ss) {
  __shared__ double sh[256];
  const double *col = Xs + (size_t)blockIdx.x * (size_t)n;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += col[i] * col[i];
  s = aq_block_sum(s, sh);
  if (threadIdx.x == 0) ss[blockIdx.x] = s;
}
