// aq_screen_tile.h -- what the f64-MFMA tile kernels of the screen family share: aq_k_ms_tile
// (aq_mscreen_kernels.h), aq_k_msperm_tile (aq_msperm_kernels.h), aq_k_cis_tile and aq_k_cis_perm_tile (aq_cis_kernels.h),
// aq_k_cc_tile (aq_ciscond_kernels.h) and aq_k_ci_tile (aq_cisint_kernels.h, on the sibling loop aq_ms_tile_loop_x2).  The tile geometry and the panel movers, the staged main loop, the pair statistic, the
// lane and wave reductions and the three small kernels every entry runs around its tile kernel exist here and nowhere else, so
// that "r of a pair is the same bits in every kernel of the family", which the GPU tests require, is a property of one text.
// A kernel header keeps its argument block, its LDS declarations, its work-item decoding and the parts of the epilogue that
// are its own.
// Several units include this header (DESIGN.md section 1 lets a header with a non-template kernel into one unit only), so
// the kernels here that are no templates are static: each unit has its own copy.
//
// Geometry.  Xs is [p1][n] and the trait side is [columns][n]: the contraction index, the sample, is the contiguous one of
// BOTH operands.  A workgroup of 256 threads owns T predictors x T trait columns (T = 64 or 128) and all n samples, which go
// through LDS AQ_MSCREEN_NC = 16 at a time as panels P[column][sample], rows of AQ_MSCREEN_STR = 18 doubles: PX of the
// predictors and NP trait-side panels (the traits; the traits of PB permutations; the residual traits and KC basis panels).
// A panel is T runs of 128 contiguous bytes of global memory, every lane taking 16 of them in one global_load_dwordx4 (A16:
// n is even, chosen by the host; two 8-byte loads when n is odd); a column beyond the matrix or a sample >= n is staged as 0.0.
// Operands: A = trait side, B = X, one f64 per lane, lane = 16 k + column (k = sample within the step of 4): lane (g, l) =
// (lane >> 4, lane & 15) reads P[(16 i + l) STR + kk + g].  The accumulator has col = lane & 15 (the predictor) and
// row = (lane >> 4) + 4 reg (the trait): the layout aq_probe_dmode verifies, which every entry requires before it launches.
// Sixteen lanes along the predictor make the dense store and the per-trait reductions run along lanes.  The four waves tile
// the output 2 x 2 (wr over traits, wc over predictors); a wave holds NI^2 = (T / 32)^2 accumulators per stream.
// LDS banks: ds_read_b64 banks by (byte address / 4) mod 64 within each half wave, i.e. by (double index) mod 32.  A half
// wave holds g in {0, 1} (or {2, 3}) and l = 0 ... 15 and reads the doubles 18 l + g + const.  18 l mod 32 = 2 (9 l mod 16),
// and 9 is odd, so l -> 9 l mod 16 is a permutation: the sixteen rows start on the sixteen even residues, g fills in the odd
// ones, and the 32 lanes hit 32 different doubles mod 32 -- no conflict.  (A row of 16 doubles would put rows l and l + 2 on
// the same banks; 17 would break the 16-byte alignment of a lane's store.  18 is even, so that store is aligned.)
//
// aq_ms_tile_loop<T, MASKED, A16, NP, GUARD, STEP>: zero the accumulators; load the first chunk of X and of the live panels into
// registers; then per chunk: barrier, registers -> LDS, barrier, load the next chunk into registers, and 4 steps of 4 samples.
// A step reads the NI operands of X once and then, panel by panel, the panel's NI operands and issues its NI^2 MFMAs.
//   MASKED = false: one stream per panel, axy += Y X.  Sx and Sxx come from aq_k_ms_colstats.
//   MASKED = true (any NaN in Yc): three streams from the same operand reads, axy += Y0 X, ax += M X, axx += M X^2,
//   with Y0 = Y with NaN replaced by 0 and M = 1.0 on observed rows, 0.0 on missing ones, both formed while the panel is
//   staged (mask panel behind the value panel), and X squared in registers.
// GUARD: the panels k >= GUARD are loaded, staged and multiplied only if k < live (`live` is uniform over the workgroup and
// >= 1), the others keep accumulators of 0.0; GUARD = NP tests none and does not read `live`.  STEP is the shape of a step
// of 4 samples: PLAIN reads X's operands and then, panel by panel, the panel's; FENCED does the same and keeps the four
// steps of a chunk apart in the schedule; PAIRED reads panel 0's operands together with X's.  Every output element is accumulated over the
// samples by one MFMA per step of 4, samples ascending, whatever T, NP, GUARD and STEP: all bit-equality between the kernels of the
// family follows from that and from aq_ms_pair.
//
// aq_ms_pair: Vx = (Sxx - Sx^2 / m) - lost, the parenthesis first; the pair is defined iff Vx > 1e-10 Sxx; r = Sxy /
// sqrt(Vx Syy).  `lost` is the variance the conditioning takes, a literal 0.0 elsewhere (x - 0.0 is x).
//
// Reductions of a trait's best predictor: per lane over its predictors in ascending order (the caller), across the sixteen
// lanes of a lane group by xor shuffles, ties in r^2 to the lowest predictor (aq_ms_lanes_best; aq_ms_lanes_max where only
// r^2 is kept), across the two waves of a tile row through LDS (aq_ms_merge_best, the lower predictors win a tie; or
// aq_ms_key_max: ONE integer atomicMax per trait and workgroup on key = bits(r^2) + 1 -- r^2 >= 0, so the order of the bit
// patterns is the order of the values, the maximum is exact and independent of the order of arrival, and key 0 says that no
// pair of the trait is defined; aq_ms_key_r2 turns a key back).
//
// aq_k_ms_traitstats, one thread per trait: Syy_t and m_t, added in index order.
// aq_k_ms_colstats, grid p1, 256 threads: Sx and Sxx of a column over all rows in the fixed order of aq_block_sum (what the
// complete instances use for every trait: m_t = n there).
// aq_k_ms_gather: Yp[b][j][i] = Yc[order[j]][perm[b][i]]; a NULL order is the identity (the plain screen's permutations), a
// NULL perm the ordered copy (the cis scans).  A workgroup writes whole columns, 256 consecutive doubles at a time
// (coalesced); its scattered reads stay inside one column of Yc, 8 n bytes that sit in L2.  NaN moves with the value: nothing
// is computed on it.  The host has checked every index of perm and built order.
#pragma once
#include "aq_mscreen_plan.h"  // AQ_MSCREEN_NC, AQ_MSCREEN_STR
#include "aq_prep_dev.h"      // aq_block_sum

typedef double aq_ms_d4 __attribute__((ext_vector_type(4)));

template <int T>
struct AqMsShape {
  static constexpr int STR = AQ_MSCREEN_STR;
  static constexpr int WT = T / 2;                         // columns per wave and operand
  static constexpr int NI = WT / 16;                       // 16-column tiles per wave and operand
  static constexpr int NV = T * (AQ_MSCREEN_NC / 2) / 256;   // 16-byte vectors per thread and panel
  static constexpr int PAN = T * STR;                      // doubles of a panel
};

static __global__ __launch_bounds__(256) void aq_k_ms_traitstats(const double *__restrict__ Yc, int n, int q, double *__restrict__ syy,
                                                                int *__restrict__ mt) {
  const int t = (int)blockIdx.x * 256 + threadIdx.x;
  if (t >= q) return;
  const double *col = Yc + (size_t)t * (size_t)n;
  double s = 0.0;
  int m = 0;
  for (int i = 0; i < n; i++) {
    const double y = col[i];
    if (y == y) {
      s += y * y;
      m++;
    }
  }
  syy[t] = s;
  mt[t] = m;
}

static __global__ __launch_bounds__(256) void aq_k_ms_colstats(const double *__restrict__ Xs, int n, double *__restrict__ sx,
                                                              double *__restrict__ sxx) {
  __shared__ double sh[256];
  const double *col = Xs + (size_t)blockIdx.x * (size_t)n;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    a += col[i];
    b += col[i] * col[i];
  }
  a = aq_block_sum(a, sh);
  b = aq_block_sum(b, sh);
  if (threadIdx.x == 0) {
    sx[blockIdx.x] = a;
    sxx[blockIdx.x] = b;
  }
}

static __global__ __launch_bounds__(256) void aq_k_ms_gather(const double *__restrict__ Yc, const int32_t *__restrict__ order,
                                                            const int32_t *__restrict__ perm, int n, int qa, int nb,
                                                            double *__restrict__ Yp) {
  const long long cols = (long long)nb * (long long)qa;
  for (long long c = blockIdx.x; c < cols; c += gridDim.x) {
    const int j = (int)(c % qa);
    const double *src = Yc + (size_t)(order ? order[j] : j) * (size_t)n;
    double *dst = Yp + (size_t)c * (size_t)n;
    if (perm) {
      const int32_t *row = perm + (size_t)(c / qa) * (size_t)n;
      for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[row[i]];
    } else {
      for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
    }
  }
}

// columns [c0, c0 + T) x samples [i0, i0 + AQ_MSCREEN_NC) of M ([ncols][n]) -> v; 0.0 for a column >= ncols and a sample >= n
// A16: n is even, so every pair starts at a multiple of 16 bytes and ends inside its column: one 16-byte load
template <int T, bool A16>
__device__ __forceinline__ void aq_ms_load(const double *__restrict__ M, int n, int ncols, int c0, int i0,
                                           double2 (&v)[AqMsShape<T>::NV]) {
#pragma unroll
  for (int u = 0; u < AqMsShape<T>::NV; u++) {
    const int idx = threadIdx.x + 256 * u;
    const int c = c0 + idx / (AQ_MSCREEN_NC / 2);
    const int s = i0 + 2 * (idx % (AQ_MSCREEN_NC / 2));
    double2 x = make_double2(0.0, 0.0);
    if (c < ncols && s < n) {
      const double *src = M + (size_t)c * (size_t)n + (size_t)s;
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
__device__ __forceinline__ void aq_ms_store(const double2 (&v)[AqMsShape<T>::NV], double *P) {
#pragma unroll
  for (int u = 0; u < AqMsShape<T>::NV; u++) {
    const int idx = threadIdx.x + 256 * u;
    *reinterpret_cast<double2 *>(P + (idx / (AQ_MSCREEN_NC / 2)) * AQ_MSCREEN_STR + 2 * (idx % (AQ_MSCREEN_NC / 2))) = v[u];
  }
}

// the panel of Y as Y0 (NaN -> 0.0) in P0 and as the mask M (1.0 observed, 0.0 missing) in PM
template <int T>
__device__ __forceinline__ void aq_ms_store_masked(const double2 (&v)[AqMsShape<T>::NV], double *P0, double *PM) {
#pragma unroll
  for (int u = 0; u < AqMsShape<T>::NV; u++) {
    const int idx = threadIdx.x + 256 * u;
    const int off = (idx / (AQ_MSCREEN_NC / 2)) * AQ_MSCREEN_STR + 2 * (idx % (AQ_MSCREEN_NC / 2));
    const bool ox = v[u].x == v[u].x, oy = v[u].y == v[u].y;
    *reinterpret_cast<double2 *>(P0 + off) = make_double2(ox ? v[u].x : 0.0, oy ? v[u].y : 0.0);
    *reinterpret_cast<double2 *>(PM + off) = make_double2(ox ? 1.0 : 0.0, oy ? 1.0 : 0.0);
  }
}

// the thread's place in the 2 x 2 waves x 4 x 16 lanes of a workgroup
struct AqMsLane {
  int lane, g, l, wr, wc;
  __device__ __forceinline__ AqMsLane()
      : lane(threadIdx.x & 63), g(lane >> 4), l(lane & 15), wr((int)(threadIdx.x >> 7)), wc((int)(threadIdx.x >> 6) & 1) {}
};

// the accumulators of NP trait-side panels: Sxy per pair, and the two sets Sx and Sxx that only MASKED has ([1][1] and never
// read otherwise).  Plain arrays of the kernel, handed to the loop by reference: wrapped in one struct the masked PB = 2
// instances spill more.
template <int T, int NP>
using aq_ms_acc = aq_ms_d4[NP][AqMsShape<T>::NI][AqMsShape<T>::NI];
template <int T, bool MASKED, int NP>
using aq_ms_acc_m = aq_ms_d4[NP][MASKED ? AqMsShape<T>::NI : 1][MASKED ? AqMsShape<T>::NI : 1];

// PX: one panel; PT: NP trait-side panels, a panel's mask (MASKED) behind its values.  base(k): panel k in global memory,
// [ncols][n], of which the tile takes the columns [c0, c0 + T).
enum { AQ_MS_STEP_PLAIN = 0, AQ_MS_STEP_FENCED = 1, AQ_MS_STEP_PAIRED = 2 };   // STEP of aq_ms_tile_loop

template <int T, bool MASKED, bool A16, int NP, int GUARD, int STEP, typename Base>
__device__ __forceinline__ void aq_ms_tile_loop(const double *Xs, int n, int p1, int p0, int ncols, int c0, int live, Base base,
                                                double *PX, double *PT, aq_ms_acc<T, NP> &axy, aq_ms_acc_m<T, MASKED, NP> &ax, aq_ms_acc_m<T, MASKED, NP> &axx) {
  typedef AqMsShape<T> SH;
  constexpr int NI = SH::NI, NS = MASKED ? NI : 1;
  constexpr int PAN = SH::PAN, TPAN = (MASKED ? 2 : 1) * PAN;
  const AqMsLane ln;
#pragma unroll
  for (int k = 0; k < NP; k++) {
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
      for (int jj = 0; jj < NI; jj++) axy[k][i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NS; i++)
#pragma unroll
      for (int jj = 0; jj < NS; jj++) {
        ax[k][i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
        axx[k][i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
      }
  }
  const int toff = (ln.wr * SH::WT + ln.l) * SH::STR + ln.g;   // the lane's first operand within a trait-side panel
  const double *px = PX + (ln.wc * SH::WT + ln.l) * SH::STR + ln.g;
  double2 vx[SH::NV], vt[NP][SH::NV];
  aq_ms_load<T, A16>(Xs, n, p1, p0, 0, vx);
#pragma unroll
  for (int k = 0; k < NP; k++)
    if (k < GUARD || k < live) aq_ms_load<T, A16>(base(k), n, ncols, c0, 0, vt[k]);
  for (int i0 = 0; i0 < n; i0 += AQ_MSCREEN_NC) {
    __syncthreads();                             // the panels of the previous chunk have been read
    aq_ms_store<T>(vx, PX);
#pragma unroll
    for (int k = 0; k < NP; k++)
      if (k < GUARD || k < live) {
        if (MASKED)
          aq_ms_store_masked<T>(vt[k], PT + k * TPAN, PT + k * TPAN + PAN);
        else
          aq_ms_store<T>(vt[k], PT + k * TPAN);
      }
    __syncthreads();
    if (i0 + AQ_MSCREEN_NC < n) {
      aq_ms_load<T, A16>(Xs, n, p1, p0, i0 + AQ_MSCREEN_NC, vx);
#pragma unroll
      for (int k = 0; k < NP; k++)
        if (k < GUARD || k < live) aq_ms_load<T, A16>(base(k), n, ncols, c0, i0 + AQ_MSCREEN_NC, vt[k]);
    }
#pragma unroll
    for (int kk = 0; kk < AQ_MSCREEN_NC; kk += 4) {
      constexpr bool PAIRED = STEP == AQ_MS_STEP_PAIRED;   // panel 0's operands are read with X's: it is never tested
      static_assert(!PAIRED || GUARD >= 1, "a panel read with X is always live");
      double x[NI], x2[NI], y[NI], m[NI];
#pragma unroll
      for (int i = 0; i < NI; i++) {
        if (PAIRED) y[i] = PT[toff + 16 * i * SH::STR + kk];
        x[i] = px[16 * i * SH::STR + kk];
        if (MASKED) {
          if (PAIRED) m[i] = PT[PAN + toff + 16 * i * SH::STR + kk];
          x2[i] = x[i] * x[i];
        }
      }
#pragma unroll
      for (int k = 0; k < NP; k++)
        if (k < GUARD || k < live) {
          if (!PAIRED || k > 0) {
            const double *pt = PT + k * TPAN + toff;
#pragma unroll
            for (int i = 0; i < NI; i++) {
              y[i] = pt[16 * i * SH::STR + kk];
              if (MASKED) m[i] = pt[PAN + 16 * i * SH::STR + kk];
            }
          }
#pragma unroll
          for (int i = 0; i < NI; i++)
#pragma unroll
            for (int jj = 0; jj < NI; jj++) {
              axy[k][i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[i], x[jj], axy[k][i][jj], 0, 0, 0);
              if (MASKED) {
                ax[k][i % NS][jj % NS] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[i], x[jj], ax[k][i % NS][jj % NS], 0, 0, 0);
                axx[k][i % NS][jj % NS] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[i], x2[jj], axx[k][i % NS][jj % NS], 0, 0, 0);
              }
            }
        }
      if (STEP == AQ_MS_STEP_FENCED) __builtin_amdgcn_sched_barrier(0);   // nothing of the next step is scheduled into this one
    }
  }
}

// The sibling of aq_ms_tile_loop for the interaction scan (aq_k_ci_tile, aq_cisint_kernels.h): complete Y, ONE trait-side
// panel and TWO predictor-side streams fed from the one staged panel of X, acc0 += Y X and acc1 += Y (X o mult), the second
// operand x * mult[sample] formed in registers with one rounding, as the masked instances above form x^2: no second LDS panel
// and no p1 x n matrix of products.  The movers, the shapes, the lane struct, the staging and the order of accumulation (one
// MFMA per step of 4 samples, samples ascending) are those of aq_ms_tile_loop, so acc0 of a pair is axy of the plain scan on
// the same panel to the bit; the operands of the one panel are read together with X's (STEP = PAIRED there).  A lane's operand
// of step kk holds sample i0 + kk + g, so its multiplier is mpad[i0 + kk + g]: mpad is the multiplier padded with zeros to
// whole chunks of AQ_MSCREEN_NC samples (aq_cisint_mult_pad), read without a guard, the four of a chunk together with the
// chunk's panels one chunk ahead.  aq_ms_tile_loop's text is not touched: its five kernels compile to the ISA they had.
template <int T, bool A16>
__device__ __forceinline__ void aq_ms_tile_loop_x2(const double *Xs, int n, int p1, int p0, const double *Yo, int ncols, int c0,
                                                   const double *__restrict__ mpad, double *PX, double *PT, aq_ms_acc<T, 1> &acc0,
                                                   aq_ms_acc<T, 1> &acc1) {
  typedef AqMsShape<T> SH;
  constexpr int NI = SH::NI, NK = AQ_MSCREEN_NC / 4;
  const AqMsLane ln;
#pragma unroll
  for (int i = 0; i < NI; i++)
#pragma unroll
    for (int jj = 0; jj < NI; jj++) {
      acc0[0][i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
      acc1[0][i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
    }
  const double *pt = PT + (ln.wr * SH::WT + ln.l) * SH::STR + ln.g;
  const double *px = PX + (ln.wc * SH::WT + ln.l) * SH::STR + ln.g;
  double2 vx[SH::NV], vt[SH::NV];
  double mnext[NK], mk[NK];
  aq_ms_load<T, A16>(Xs, n, p1, p0, 0, vx);
  aq_ms_load<T, A16>(Yo, n, ncols, c0, 0, vt);
#pragma unroll
  for (int s = 0; s < NK; s++) mnext[s] = mpad[4 * s + ln.g];
  for (int i0 = 0; i0 < n; i0 += AQ_MSCREEN_NC) {
    __syncthreads();                             // the panels of the previous chunk have been read
    aq_ms_store<T>(vx, PX);
    aq_ms_store<T>(vt, PT);
#pragma unroll
    for (int s = 0; s < NK; s++) mk[s] = mnext[s];
    __syncthreads();
    if (i0 + AQ_MSCREEN_NC < n) {                // then i0 + 2 AQ_MSCREEN_NC <= the length of mpad
      aq_ms_load<T, A16>(Xs, n, p1, p0, i0 + AQ_MSCREEN_NC, vx);
      aq_ms_load<T, A16>(Yo, n, ncols, c0, i0 + AQ_MSCREEN_NC, vt);
#pragma unroll
      for (int s = 0; s < NK; s++) mnext[s] = mpad[i0 + AQ_MSCREEN_NC + 4 * s + ln.g];
    }
#pragma unroll
    for (int kk = 0; kk < AQ_MSCREEN_NC; kk += 4) {
      double x[NI], xm[NI], y[NI];
#pragma unroll
      for (int i = 0; i < NI; i++) {
        y[i] = pt[16 * i * SH::STR + kk];
        x[i] = px[16 * i * SH::STR + kk];
        xm[i] = x[i] * mk[kk / 4];               // one rounding
      }
#pragma unroll
      for (int i = 0; i < NI; i++)
#pragma unroll
        for (int jj = 0; jj < NI; jj++) {
          acc0[0][i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[i], x[jj], acc0[0][i][jj], 0, 0, 0);
          acc1[0][i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[i], xm[jj], acc1[0][i][jj], 0, 0, 0);
        }
    }
  }
}

// ts[i] = src[j0 + i] for the tile's trait column i = threadIdx.x < T, 0 for a column >= count: the callers fill all their
// arrays under one `if ((int)threadIdx.x < T)`.  Read after the loop's barriers.
template <int T, typename V>
__device__ __forceinline__ void aq_ms_trait_fill(V (&ts)[T], const V *__restrict__ src, int j0, int count) {
  ts[threadIdx.x] = j0 + (int)threadIdx.x < count ? src[j0 + (int)threadIdx.x] : V(0);
}

// Sx and Sxx of the lane's NI predictors s0 + 16 jj for the complete instances (USE), 0.0 otherwise and for s >= p1
template <int NI, bool USE>
__device__ __forceinline__ void aq_ms_col_sums(const double *__restrict__ sx, const double *__restrict__ sxx, int s0, int p1, double (&csx)[NI],
                                               double (&csxx)[NI]) {
#pragma unroll
  for (int jj = 0; jj < NI; jj++) {
    const int s = s0 + 16 * jj;
    csx[jj] = (USE && s < p1) ? sx[s] : 0.0;
    csxx[jj] = (USE && s < p1) ? sxx[s] : 0.0;
  }
}

// the pair statistic: whether the pair is defined, and then *r
__device__ __forceinline__ bool aq_ms_pair(double sxy, double sx, double sxx, double m, double syy, double lost, double *r) {
  const double vx0 = sxx - sx * sx / m;
  const double vx = vx0 - lost;
  const bool ok = vx > 1e-10 * sxx;
  if (ok) *r = sxy / sqrt(vx * syy);
  return ok;
}

// the best (r^2, r, predictor) of a trait across the sixteen lanes of the lane group: ties to the lowest predictor
__device__ __forceinline__ void aq_ms_lanes_best(double &br2, double &br, int &bs) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
    const double o2 = __shfl_xor(br2, off), orr = __shfl_xor(br, off);
    const int os = __shfl_xor(bs, off);
    const bool take = o2 > br2 || (o2 == br2 && os < bs);   // selects, not a branch around three moves
    br2 = take ? o2 : br2;
    br = take ? orr : br;
    bs = take ? os : bs;
  }
}

__device__ __forceinline__ double aq_ms_lanes_max(double br2) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
    const double o2 = __shfl_xor(br2, off);
    if (o2 > br2) br2 = o2;
  }
  return br2;
}

// a count summed over the lanes [from, to) of xor distance: (1, 16) the sixteen lanes of a lane group, (16, 64) the four lane
// groups, (1, 64) the wave
template <typename V>
__device__ __forceinline__ V aq_ms_lanes_sum(V c, int from, int to) {
#pragma unroll
  for (int off = from; off < to; off <<= 1) c += __shfl_xor(c, off);
  return c;
}

// the candidates (r, predictor; 0x7fffffff: none) of the two waves of a tile row -> part[o]: the lower predictors win a tie
template <int T>
__device__ __forceinline__ void aq_ms_merge_best(const double (&cand_r)[2][T], const int (&cand_s)[2][T], int tl, double *part_r,
                                                 int32_t *part_s, size_t o) {
  double r = cand_r[0][tl];
  int s = cand_s[0][tl];
  const double r1 = cand_r[1][tl];
  const int s1 = cand_s[1][tl];
  if (s1 != 0x7fffffff && (s == 0x7fffffff || r1 * r1 > r * r)) {
    r = r1;
    s = s1;
  }
  part_r[o] = r;
  part_s[o] = s == 0x7fffffff ? -1 : s;
}

// the largest r^2 (-1.0: none) of the two waves of a tile row -> the trait's key
__device__ __forceinline__ void aq_ms_key_max(double m0, double m1, unsigned long long *key) {
  const double m = m1 > m0 ? m1 : m0;
  if (m >= 0.0) atomicMax(key, (unsigned long long)__double_as_longlong(m) + 1ull);
}

__device__ __forceinline__ double aq_ms_key_r2(unsigned long long k) {
  return k ? __longlong_as_double((long long)(k - 1ull)) : -1.0;
}
