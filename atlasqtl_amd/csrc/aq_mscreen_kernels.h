// aq_mscreen_kernels.h -- the marginal screen of a finished prepare handle: the correlation of
// every predictor (column of Xs) with every trait (column of Yc) over the trait's observed rows, on the f64 matrix pipe, and
// what is read off it in registers: the selected pairs, the per-predictor counts, each trait's best predictor.  Included by
// aq_prep_marginal.hip; the launch plan is aq_mscreen_plan.h.  Every kernel is a plain grid: no workgroup waits for another
// one, nothing spins, and no floating-point atomic is used (the integer atomics are counters), so two calls on one handle
// give the same set of rows and the same bits everywhere else.
//
// The statistic (include/atlasqtl_hip.h, aq_prep_marginal).  For predictor s and trait t, over the m_t observed rows O_t of
// the trait: Sxy = sum x y, Sx = sum x, Sxx = sum x^2, Syy_t = sum y^2; Vx = Sxx - Sx^2 / m_t; r = Sxy / sqrt(Vx Syy_t);
// df_t = m_t - 2 - n_cov.  The pair is undefined (r = NaN, never selected, counted) when Vx <= 1e-10 Sxx, Syy_t = 0 or df_t < 1.
//
// Xs is [p1][n] and Yc is [q][n]: the contraction index, the sample, is the contiguous one of BOTH operands.
//
// aq_k_ms_traitstats, one thread per trait: Syy_t and m_t, added in index order.
// aq_k_ms_colstats, grid p1, 256 threads: Sx and Sxx of a column over all rows in the fixed order of aq_block_sum (what the
// complete instance uses for every trait: m_t = n there).
//
// aq_k_ms_tile<T, MASKED, A16>, grid n_tiles, 256 threads; A16 = n is even, chosen by the host as for aq_k_grm_partial.
// Workgroup b owns predictors [T tp, T tp + T) x traits [T tq, T tq + T), (tp, tq) = (b mod tiles_p, b / tiles_p), and all n
// samples, which go through LDS AQ_MSCREEN_NC = 16 at a time as panels P[column][sample]: PX of the predictors, PY of the
// traits, rows of AQ_MSCREEN_STR = 18 doubles.  A panel is T runs of 128 contiguous bytes of global memory, every lane
// taking 16 of them in one global_load_dwordx4 (A16; two 8-byte loads when n is odd: a template argument, as in aq_grm_load);
// a column >= p1 (q) or a sample >= n is staged as 0.0.  The next chunk is loaded into registers before the current one is
// multiplied.
// Operands: A = Y, B = X, one f64 per lane, lane = 16 k + column (k = sample within the step of 4): lane (g, l) =
// (lane >> 4, lane & 15) reads P[(16 i + l) STR + kk + g].  The accumulator has col = lane & 15 (the predictor) and
// row = (lane >> 4) + 4 reg (the trait): the layout aq_probe_dmode verifies, which aq_prep_marginal requires before it
// launches.  Sixteen lanes along the predictor make the dense store and the per-trait reduction run along lanes.
// LDS banks: ds_read_b64 banks by (byte address / 4) mod 64 within each half wave, i.e. by (double index) mod 32.  A half
// wave holds g in {0, 1} (or {2, 3}) and l = 0 ... 15 and reads the doubles 18 l + g + const.  18 l mod 32 = 2 (9 l mod 16),
// and 9 is odd, so l -> 9 l mod 16 is a permutation: the sixteen rows start on the sixteen even residues, g fills in the odd
// ones, and the 32 lanes hit 32 different doubles mod 32 -- no conflict.  (A row of 16 doubles would put rows l and l + 2 on
// the same banks; 17 would break the 16-byte alignment of a lane's store.  18 is even, so that store is aligned.)
// The four waves tile the output 2 x 2 (wr over traits, wc over predictors); a wave holds (T / 32)^2 accumulators per
// stream and per step of 4 samples issues T / 32 LDS reads of each operand.
//   MASKED = false (Yc complete): one stream, acc_xy += Y X.  Sx and Sxx come from aq_k_ms_colstats.
//   MASKED = true (any NaN in Yc): three streams from the same operand reads, acc_xy += Y0 X, acc_x += M X, acc_xx += M X^2,
//   with Y0 = Y with NaN replaced by 0 and M = 1.0 on observed rows, 0.0 on missing ones, both formed while the panel of Y is
//   staged (PY and PM), and X squared in registers.  Three accumulator sets at T = 128 would take 384 registers, so this
//   instance exists at T = 64 only (96).
// Two workgroups share a CU (__launch_bounds__(256, 2): at most 256 registers a lane), so one stages or runs its epilogue
// while the other multiplies.
// Epilogue, in registers: r by the definition above, the tile's Syy_t, m_t and cutoffs from LDS (read from global memory once
// per workgroup, before the loop) and the complete instance's Sx, Sxx of the lane's predictors from registers; then
//   - a selected pair (r^2 >= r2_cut[t]) takes a slot from one 64-bit integer counter, which keeps counting beyond cap, and
//     writes (snp, trait, r) there if slot < cap; the order of the rows is unspecified, their set is not;
//   - the per-predictor count of selected traits: summed over the lane's traits, then over the four lane groups, then one
//     integer atomic per predictor and wave;
//   - undefined pairs: counted per wave, one integer atomic;
//   - each trait's best predictor by r^2 within the tile, ties to the lowest predictor index: per lane over its
//     predictors in ascending order, across the sixteen lanes by xor shuffles with the tie rule, across the two waves of a
//     tile row through LDS, then to part[tp][t]; aq_k_ms_best walks tp = 0, 1, ... and takes a later tile only if it is
//     strictly better;
//   - the dense r, if asked for: r_dense[t p1 + s], 16 lanes writing 128 consecutive bytes.
#pragma once
#include "aq_mscreen_plan.h"
#include "aq_prep_dev.h"      // aq_block_sum

typedef double aq_ms_d4 __attribute__((ext_vector_type(4)));

struct aq_ms_args {
  const double *Xs, *Yc;              // [p1][n], [q][n]
  int n, p1, q, n_cov, tiles_p;
  const double *sx, *sxx;             // p1 each: the complete instance's Sx and Sxx
  const double *syy;                  // q
  const int *mt;                      // q
  const double *cut;                  // q: the cutoff on r^2
  int32_t *snp, *trait;               // cap rows
  double *r;
  long long cap;
  unsigned long long *n_pairs, *n_undef, *rs;   // two counters; p1 counts
  double *part_r;                     // [tiles_p][q]: r of the tile row's best predictor (NaN: none)
  int32_t *part_s;                    // [tiles_p][q]: that predictor (-1: none)
  double *r_dense;                    // nullptr, or [q][p1]
};

template <int T>
struct AqMsShape {
  static constexpr int STR = AQ_MSCREEN_STR;
  static constexpr int WT = T / 2;                         // columns per wave and operand
  static constexpr int NI = WT / 16;                       // 16-column tiles per wave and operand
  static constexpr int NV = T * (AQ_MSCREEN_NC / 2) / 256;   // 16-byte vectors per thread and panel
};

// the kernels that are no templates are static: two units include this header (aq_prep_marginal.hip, aq_prep_marginal_perm.hip)
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

template <int T, bool MASKED, bool A16>
__global__ __launch_bounds__(256, 2) void aq_k_ms_tile(const aq_ms_args a) {
  typedef AqMsShape<T> SH;
  constexpr int NS = MASKED ? SH::NI : 1;                  // extent of the two extra accumulator sets (1: unused)
  __shared__ __attribute__((aligned(16))) double PX[T * SH::STR];
  __shared__ __attribute__((aligned(16))) double PYM[(MASKED ? 2 : 1) * T * SH::STR];
  double *const PY = PYM, *const PM = PYM + (MASKED ? T * SH::STR : 0);   // PM is read and written by the masked instance only
  __shared__ double cand_r[2][T];
  __shared__ int cand_s[2][T];
  __shared__ double ts_syy[T], ts_cut[T];                  // the tile's traits: Syy_t, the cutoff, and m_t (0 for a trait >= q)
  __shared__ int ts_m[T];
  static_assert(sizeof(double) * ((MASKED ? 3 : 2) * T * SH::STR) + 2 * T * 12 + T * 20 == aq_mscreen_lds_bytes(T, MASKED), "plan and kernel");
  static_assert(aq_mscreen_lds_bytes(T, MASKED) <= 65536, "64 KB of static LDS");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, l = lane & 15;
  const int wr = w >> 1, wc = w & 1;
  const int tp = (int)(blockIdx.x % (unsigned)a.tiles_p), tq = (int)(blockIdx.x / (unsigned)a.tiles_p);
  const int p0 = T * tp, q0 = T * tq;
  const int n = a.n;
  aq_ms_d4 axy[SH::NI][SH::NI], ax[NS][NS], axx[NS][NS];
#pragma unroll
  for (int i = 0; i < SH::NI; i++)
#pragma unroll
    for (int jj = 0; jj < SH::NI; jj++) axy[i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < NS; i++)
#pragma unroll
    for (int jj = 0; jj < NS; jj++) {
      ax[i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
      axx[i][jj] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
    }
  const double *py = PY + (wr * SH::WT + l) * SH::STR + g;
  const double *pm = PM + (wr * SH::WT + l) * SH::STR + g;
  const double *px = PX + (wc * SH::WT + l) * SH::STR + g;
  if ((int)threadIdx.x < T) {                      // read after the loop's barriers
    const int t = q0 + (int)threadIdx.x;
    const bool tv = t < a.q;
    ts_syy[threadIdx.x] = tv ? a.syy[t] : 0.0;
    ts_cut[threadIdx.x] = tv ? a.cut[t] : 0.0;
    ts_m[threadIdx.x] = tv ? a.mt[t] : 0;
  }
  double2 vx[SH::NV], vy[SH::NV];
  aq_ms_load<T, A16>(a.Xs, n, a.p1, p0, 0, vx);
  aq_ms_load<T, A16>(a.Yc, n, a.q, q0, 0, vy);
  for (int i0 = 0; i0 < n; i0 += AQ_MSCREEN_NC) {
    __syncthreads();                             // the panels of the previous chunk have been read
    aq_ms_store<T>(vx, PX);
    if (MASKED)
      aq_ms_store_masked<T>(vy, PY, PM);
    else
      aq_ms_store<T>(vy, PY);
    __syncthreads();
    if (i0 + AQ_MSCREEN_NC < n) {
      aq_ms_load<T, A16>(a.Xs, n, a.p1, p0, i0 + AQ_MSCREEN_NC, vx);
      aq_ms_load<T, A16>(a.Yc, n, a.q, q0, i0 + AQ_MSCREEN_NC, vy);
    }
#pragma unroll
    for (int kk = 0; kk < AQ_MSCREEN_NC; kk += 4) {
      double y[SH::NI], m[SH::NI], x[SH::NI], x2[SH::NI];
#pragma unroll
      for (int i = 0; i < SH::NI; i++) {
        y[i] = py[16 * i * SH::STR + kk];
        x[i] = px[16 * i * SH::STR + kk];
        if (MASKED) {
          m[i] = pm[16 * i * SH::STR + kk];
          x2[i] = x[i] * x[i];
        }
      }
#pragma unroll
      for (int i = 0; i < SH::NI; i++)
#pragma unroll
        for (int jj = 0; jj < SH::NI; jj++) {
          axy[i][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[i], x[jj], axy[i][jj], 0, 0, 0);
          if (MASKED) {
            ax[i % NS][jj % NS] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[i], x[jj], ax[i % NS][jj % NS], 0, 0, 0);
            axx[i % NS][jj % NS] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[i], x2[jj], axx[i % NS][jj % NS], 0, 0, 0);
          }
        }
    }
  }

  // ---- epilogue: r of the wave's (T / 2)^2 pairs, four traits (g + 4 reg) x one predictor (l) per accumulator and lane ----
  unsigned long long undef = 0;
  unsigned int sel[SH::NI];
  double csx[SH::NI], csxx[SH::NI];                // the complete instance's Sx and Sxx of the lane's predictors
#pragma unroll
  for (int jj = 0; jj < SH::NI; jj++) {
    sel[jj] = 0;
    const int s = p0 + wc * SH::WT + 16 * jj + l;
    csx[jj] = (!MASKED && s < a.p1) ? a.sx[s] : 0.0;
    csxx[jj] = (!MASKED && s < a.p1) ? a.sxx[s] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < SH::NI; i++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int tl = wr * SH::WT + 16 * i + g + 4 * reg, t = q0 + tl;
      const bool tv = t < a.q;
      const double syy = ts_syy[tl], cut = ts_cut[tl];
      const int m = ts_m[tl];
      const double md = (double)m;
      const bool t_ok = tv && m - 2 - a.n_cov >= 1 && syy > 0.0;
      double br2 = -1.0, br = __builtin_nan("");
      int bs = 0x7fffffff;
#pragma unroll
      for (int jj = 0; jj < SH::NI; jj++) {
        const int s = p0 + wc * SH::WT + 16 * jj + l;
        if (tv && s < a.p1) {
          double r = __builtin_nan("");
          bool ok = false;
          if (t_ok) {
            const double sxy = axy[i][jj][reg];
            const double sx = MASKED ? ax[i % NS][jj % NS][reg] : csx[jj];
            const double sxx = MASKED ? axx[i % NS][jj % NS][reg] : csxx[jj];
            const double vx = sxx - sx * sx / md;
            ok = vx > 1e-10 * sxx;
            if (ok) r = sxy / sqrt(vx * syy);
          }
          if (ok) {
            const double r2 = r * r;
            if (r2 >= cut) {
              sel[jj]++;
              const unsigned long long slot = atomicAdd(a.n_pairs, 1ull);
              if ((long long)slot < a.cap) {
                a.snp[slot] = s;
                a.trait[slot] = t;
                a.r[slot] = r;
              }
            }
            if (r2 > br2) {                        // ascending s: the first of equal r^2 stays
              br2 = r2;
              br = r;
              bs = s;
            }
          } else {
            undef++;
          }
          if (a.r_dense) a.r_dense[(size_t)t * (size_t)a.p1 + (size_t)s] = r;
        }
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {     // across the sixteen predictors of the lane group
        const double o2 = __shfl_xor(br2, off), orr = __shfl_xor(br, off);
        const int os = __shfl_xor(bs, off);
        if (o2 > br2 || (o2 == br2 && os < bs)) {
          br2 = o2;
          br = orr;
          bs = os;
        }
      }
      if (l == 0) {
        cand_r[wc][tl] = br;
        cand_s[wc][tl] = bs;
      }
    }
#pragma unroll
  for (int jj = 0; jj < SH::NI; jj++) {            // the predictor's selected traits over the wave's T / 2 traits
    unsigned int c = sel[jj];
    c += __shfl_xor(c, 16);
    c += __shfl_xor(c, 32);
    const int s = p0 + wc * SH::WT + 16 * jj + l;
    if (g == 0 && c > 0 && s < a.p1) atomicAdd(a.rs + s, (unsigned long long)c);
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) undef += __shfl_xor(undef, off);
  if (lane == 0 && undef > 0) atomicAdd(a.n_undef, undef);
  __syncthreads();
  if ((int)threadIdx.x < T && q0 + (int)threadIdx.x < a.q) {   // the two waves of a tile row: the lower predictors win a tie
    const int tl = threadIdx.x;
    double r = cand_r[0][tl];
    int s = cand_s[0][tl];
    const double r1 = cand_r[1][tl];
    const int s1 = cand_s[1][tl];
    if (s1 != 0x7fffffff && (s == 0x7fffffff || r1 * r1 > r * r)) {
      r = r1;
      s = s1;
    }
    const size_t o = (size_t)tp * (size_t)a.q + (size_t)(q0 + tl);
    a.part_r[o] = r;
    a.part_s[o] = s == 0x7fffffff ? -1 : s;
  }
}

// each trait's best predictor over the rows of tiles, in the order tp = 0, 1, ...: a later one only if strictly better
static __global__ __launch_bounds__(256) void aq_k_ms_best(const double *__restrict__ part_r, const int32_t *__restrict__ part_s, int tiles_p,
                                                          int q, int32_t *__restrict__ best_snp, double *__restrict__ best_r) {
  const int t = (int)blockIdx.x * 256 + threadIdx.x;
  if (t >= q) return;
  double br = __builtin_nan(""), b2 = -1.0;
  int bs = -1;
  for (int tp = 0; tp < tiles_p; tp++) {
    const int s = part_s[(size_t)tp * q + t];
    const double r = part_r[(size_t)tp * q + t];
    if (s >= 0 && r * r > b2) {
      b2 = r * r;
      br = r;
      bs = s;
    }
  }
  best_snp[t] = bs;
  best_r[t] = br;
}
