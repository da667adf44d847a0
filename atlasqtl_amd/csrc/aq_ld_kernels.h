// aq_ld_kernels.h -- LD pruning of the device-side preparation: the banded correlation matrix of the
// compact standardised X on the f64 matrix pipe, the first-one-wins scan over its thresholded bits, the r^2 of every removed
// column with its tag, and the gather of the kept columns.  Included by aq_prep_ld.hip.  Every kernel is a plain grid: no
// workgroup waits for another one, nothing spins.
//
// Xs is [p1][n], every column contiguous, mean 0 and sum of squares n - 1, so r(i, j) = (Xs_i . Xs_j) / (n - 1).  Entry
// (j, b) of the band is the pair (i, j) with i = j - 1 - b, 0 <= b < window.
//
// Tiling of aq_k_ld_band.  Workgroup (mj, d) owns, for the 64 columns j = 64 mj + jl, the 64 band entries b = 64 d + b':
// one whole 64-bit word of each column's bit row, so the words are written by ordinary stores and by nobody else.  Those
// pairs lie in the 128 columns i = 64 (mj - d - 1) + il with il = jl + 63 - b' in [jl, jl + 63].  Samples go through LDS
// AQ_LD_KC at a time: a 64-column j panel and a 128-column i panel, read from global memory with every lane taking 16
// consecutive bytes of one column (8 when n is odd and the columns are not 16-byte aligned) and 16 lanes a 256-byte run.
// Wave w holds j-tile w (16 columns) and accumulates it against the five i-tiles w ... w + 4 that its parallelogram touches:
// one LDS read of B and five of A per five v_mfma_f64_16x16x4_f64.  X is therefore streamed once per 64 columns and 64 band
// entries, 192 n doubles for 4096 pairs, and 5 / 4 of the band's flops are issued.
// Operands: A and B hold one f64 per lane, lane = 16 k + column (k = sample within the step of 4); the accumulator has
// col = lane & 15 (the B column, j) and row = (lane >> 4) + 4 reg (the A column, i): the layout aq_probe_dmode verifies on
// the device, which aq_prep_ld_prune / aq_prep_ld_band require before they launch.
// LDS rows are AQ_LD_S = 34 doubles: even, so a lane's 16-byte store is aligned, and 34 i + k over a half wave (16 columns,
// k = 0, 1) hits 32 different 8-byte banks.
#pragma once

#define AQ_LD_MAX_WINDOW 4096   // 64 words of 64 bits: one per lane of the scan's wave
#define AQ_LD_KC 32             // samples staged in LDS per step
#define AQ_LD_S 34              // doubles per column in LDS
#define AQ_LD_NT 5              // i-tiles a wave accumulates

typedef double aq_ld_d4 __attribute__((ext_vector_type(4)));

// columns [c0, c0 + ncols) x samples [k0, k0 + AQ_LD_KC) of Xs -> P[col][AQ_LD_S]; 0.0 for a column outside [0, p1) and for
// a sample >= n (the zero-filled K tail)
__device__ __forceinline__ void aq_ld_stage(const double *__restrict__ Xs, long long c0, int ncols, int p1, int n, int k0,
                                            bool aligned16, double *P) {
  for (int idx = threadIdx.x; idx < ncols * (AQ_LD_KC / 2); idx += 256) {
    const int col = idx >> 4, kk = 2 * (idx & 15), k = k0 + kk;
    const long long c = c0 + col;
    double2 v = make_double2(0.0, 0.0);
    if (c >= 0 && c < p1 && k < n) {
      const double *src = Xs + (size_t)c * (size_t)n + (size_t)k;
      if (aligned16) {                         // n even: k + 1 < n, and the address is a multiple of 16
        v = *reinterpret_cast<const double2 *>(src);
      } else {
        v.x = src[0];
        if (k + 1 < n) v.y = src[1];
      }
    }
    *reinterpret_cast<double2 *>(P + col * AQ_LD_S + kk) = v;
  }
}

// BITS = false: band[b p1 + j] = r(j - 1 - b, j), NaN where j - 1 - b < 0 (p1 x window, column-major)
// BITS = true:  bit b of column j's row (nw = ceil(window / 64) words at bits[j nw]) = the pair is eligible and r^2 > r2;
//               group (p1 entries) and pos (p1 entries, read when window_bp > 0) may be NULL
// grid (ceil(p1 / 64), ceil(window / 64)), 256 threads
template <bool BITS>
__global__ __launch_bounds__(256) void aq_k_ld_band(const double *__restrict__ Xs, int n, int p1, int window, double r2,
                                                   const int32_t *__restrict__ group, const long long *__restrict__ pos,
                                                   long long window_bp, double *__restrict__ band,
                                                   unsigned long long *__restrict__ bits, int nw) {
  __shared__ double PJ[64 * AQ_LD_S];
  __shared__ double PI[128 * AQ_LD_S];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4;
  const int mj = blockIdx.x, d = blockIdx.y;
  const long long J0 = 64ll * mj, I0 = 64ll * ((long long)mj - d - 1);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (d > mj) {                                // every i of this workgroup is negative
    if (BITS) {
      const long long j = J0 + threadIdx.x;
      if (threadIdx.x < 64 && j < p1) bits[(size_t)j * nw + d] = 0ull;
    } else {
      const long long j = J0 + lane;
      for (int bp = w; bp < 64; bp += 4) {
        const long long b = 64ll * d + bp;
        if (j < p1 && b < window) band[(size_t)b * p1 + j] = nan;
      }
    }
    return;
  }
  const int jl = 16 * w + (lane & 15);
  const long long j = J0 + jl;
  const bool aligned16 = (n & 1) == 0;
  aq_ld_d4 acc[AQ_LD_NT];
#pragma unroll
  for (int t = 0; t < AQ_LD_NT; t++) acc[t] = aq_ld_d4{0.0, 0.0, 0.0, 0.0};
  const double *pb = PJ + jl * AQ_LD_S + g;
  const double *pa = PI + jl * AQ_LD_S + g;    // i-tile w + t: + 16 t columns
  for (int k0 = 0; k0 < n; k0 += AQ_LD_KC) {
    __syncthreads();
    aq_ld_stage(Xs, J0, 64, p1, n, k0, aligned16, PJ);
    aq_ld_stage(Xs, I0, 128, p1, n, k0, aligned16, PI);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < AQ_LD_KC; kk += 4) {
      const double b = pb[kk];
#pragma unroll
      for (int t = 0; t < AQ_LD_NT; t++)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[16 * t * AQ_LD_S + kk], b, acc[t], 0, 0, 0);
    }
  }
  const double nm1 = (double)(n - 1);
  const int gj = (BITS && group && j < p1) ? group[j] : 0;
  const long long pj = (BITS && window_bp > 0 && j < p1) ? pos[j] : 0;
  unsigned long long word = 0ull;
#pragma unroll
  for (int t = 0; t < AQ_LD_NT; t++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int il = 16 * (w + t) + g + 4 * reg;
      const int bp = jl + 63 - il;
      if (bp < 0 || bp > 63) continue;
      const long long b = 64ll * d + bp, i = I0 + il;
      if (b >= window || j >= p1) continue;
      const double r = acc[t][reg] / nm1;
      if (BITS) {
        bool on = i >= 0 && r * r > r2;
        if (on && group) on = group[i] == gj;
        if (on && window_bp > 0) {
          const long long dist = pj - pos[i];
          on = (dist < 0 ? -dist : dist) <= window_bp;
        }
        if (on) word |= 1ull << bp;
      } else {
        band[(size_t)b * p1 + j] = i >= 0 ? r : nan;
      }
    }
  if (BITS) {                                  // the four lanes of a column hold disjoint bits of its word
    word |= __shfl_xor(word, 16, 64);
    word |= __shfl_xor(word, 32, 64);
    if (g == 0 && j < p1) bits[(size_t)j * nw + d] = word;
  }
}

// The greedy rule over the bit rows, one wave: lane l holds word l of the sliding window of KEPT columns (bit b = column
// j - 1 - b is kept).  Column j is removed iff its row meets the window; its tag is the smallest such i, the highest set bit
// of the highest lane.  The rows do not depend on the scan, so AQ_LD_PF of them are loaded while the previous ones are used.
#define AQ_LD_PF 8
__global__ __launch_bounds__(64) void aq_k_ld_scan(const unsigned long long *__restrict__ bits, int p1, int nw,
                                                  uint8_t *__restrict__ bool_ld, int32_t *__restrict__ ld_of) {
  const int lane = threadIdx.x;
  unsigned long long kept = 0ull, cur[AQ_LD_PF], nxt[AQ_LD_PF];
#pragma unroll
  for (int u = 0; u < AQ_LD_PF; u++) cur[u] = (lane < nw && u < p1) ? bits[(size_t)u * nw + lane] : 0ull;
  for (int j0 = 0; j0 < p1; j0 += AQ_LD_PF) {
#pragma unroll
    for (int u = 0; u < AQ_LD_PF; u++) {
      const long long jn = (long long)j0 + AQ_LD_PF + u;
      nxt[u] = (lane < nw && jn < p1) ? bits[(size_t)jn * nw + lane] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < AQ_LD_PF; u++) {
      const int j = j0 + u;
      if (j < p1) {
        const unsigned long long hit = cur[u] & kept;
        const unsigned long long ball = __ballot(hit != 0ull);
        int tag = -1;
        if (ball) {
          const int hl = 63 - __clzll((long long)ball);
          const unsigned long long hv = __shfl(hit, hl, 64);
          tag = j - 1 - (64 * hl + 63 - __clzll((long long)hv));
        }
        unsigned long long carry = __shfl_up(kept, 1, 64) >> 63;
        if (lane == 0) carry = ball ? 0ull : 1ull;
        kept = (kept << 1) | carry;
        if (lane == 0) {
          bool_ld[j] = ball ? 1 : 0;
          ld_of[j] = tag;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < AQ_LD_PF; u++) cur[u] = nxt[u];
  }
}

// s + c <- (s + c) + (s2 + c2), the rounding error of the sum kept in c
__device__ __forceinline__ void aq_ld_two_sum(double &s, double &c, double s2, double c2) {
  const double t = __dadd_rn(s, s2);
  const double bb = __dadd_rn(t, -s);
  const double err = __dadd_rn(__dadd_rn(s, -__dadd_rn(t, -bb)), __dadd_rn(s2, -bb));
  s = t;
  c = __dadd_rn(__dadd_rn(c, c2), err);
}

// ld_r2[j] = r(ld_of[j], j)^2 for a removed column, NaN otherwise.  One workgroup per column; the dot product is carried as
// an unevaluated sum of two doubles (exact products by fma, error-free additions), so r is the correctly rounded quotient
// of a sum good to about 2^-100 and r^2 is good to a few units of 2^-53.
__global__ __launch_bounds__(256) void aq_k_ld_tag_r2(const double *__restrict__ Xs, int n, const int32_t *__restrict__ ld_of,
                                                     double *__restrict__ ld_r2) {
  __shared__ double shs[256], shc[256];
  const int t = threadIdx.x, j = blockIdx.x, i = ld_of[j];
  if (i < 0) {
    if (t == 0) ld_r2[j] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const double *xi = Xs + (size_t)i * n, *xj = Xs + (size_t)j * n;
  double s = 0.0, c = 0.0;
  for (int k = t; k < n; k += 256) {
    const double x = xi[k], y = xj[k];
    const double pr = __dmul_rn(x, y);
    aq_ld_two_sum(s, c, pr, __fma_rn(x, y, -pr));
  }
  shs[t] = s;
  shc[t] = c;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (t < st) {
      double a = shs[t], b = shc[t];
      aq_ld_two_sum(a, b, shs[t + st], shc[t + st]);
      shs[t] = a;
      shc[t] = b;
    }
    __syncthreads();
  }
  if (t == 0) {
    const double r = __dadd_rn(shs[0], shc[0]) / (double)(n - 1);
    ld_r2[j] = r * r;
  }
}

// column j of src -> column dst[j] of out (skipped when dst[j] < 0): a copy of the bits
__global__ __launch_bounds__(256) void aq_k_ld_gather(const double *__restrict__ src, int n, const int32_t *__restrict__ dst,
                                                     double *__restrict__ out) {
  const int d = dst[blockIdx.x];
  if (d < 0) return;
  const double *s = src + (size_t)blockIdx.x * n;
  double *o = out + (size_t)d * n;
  for (int k = threadIdx.x; k < n; k += 256) o[k] = s[k];
}
