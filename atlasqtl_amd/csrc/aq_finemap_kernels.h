// aq_finemap_kernels.h -- cis fine-mapping of a finished prepare handle: per trait the SuSiE model
// (sum of L single effects) over the predictors of its own window, fitted by IBSS on the handle's own matrices, susieR's
// susie(standardize = FALSE, intercept = FALSE) with the EM update of the prior variances; the model is stated in
// include/atlasqtl_hip.h (aq_prep_cis_finemap).  Included by aq_prep_cis_finemap.hip alone; the launch plan is
// aq_finemap_plan.h, the order of the traits and the work items those of aq_cis_plan.h.  Every kernel is a plain grid: no
// workgroup waits for another one, nothing spins, no floating-point atomic is used (the one integer atomic is the counter of
// the rows) and every sum runs in a fixed order, so two calls give the same set of rows and the same bits everywhere else.
//
// IBSS is a Gauss-Seidel loop over the L effects, and per effect it needs x'r over the window and X b from the updated
// coefficients.  For the 64 traits of a trait tile in lockstep both are dense products: the first is the cis tile loop with the
// current residuals in the place of the traits, the second its banded transpose.  All traits of a batch (consecutive trait
// tiles, aq_finemap_plan.h) step together: per effect l one launch each of aq_k_fm_xtr, aq_k_fm_ser and aq_k_fm_fit, per
// iteration one of aq_k_fm_iter_end, which clears act[j] of a trait that has converged.  A trait with act[j] = 0 is written by
// no kernel: its state stays what it was in the iteration in which it stopped.  The host drops the tiles without an active
// trait from the two lists the grids are taken from.
//
// Per batch, with Wb its work items (slot = w - w0) and qb its ordered traits (jb = j - j0):
//   Z[slot][trait][predictor]        x_s' r_l of every pair of the item, the band buffer
//   A, M[l][slot][trait][predictor]  alpha and mu of effect l: the state.  The predictor is the contiguous index: a workgroup
//                                    of aq_k_fm_ser walks its trait's row of every item, 512 contiguous bytes each, reading
//                                    Z and writing A and M; a lane of aq_k_fm_fit reads 128 contiguous bytes of a row
//   R, Rf[jb][n], fit[l][jb][n]      the panel r_l that the tile loop reads, the running residual, the fits
// Per ordered trait j (all batches): act, P (predictors with prior weight), sig2, V[l][j], and what the ELBO needs.
//
// aq_k_fm_xtr<A16>, grid = the active items, 256 threads: the complete-Y loop of aq_screen_tile.h with one trait-side panel,
// R, over work item w = act_items[blockIdx.x]; the epilogue stores the raw accumulators, sixteen lanes along the predictor.
// aq_k_fm_ser, grid qb, 256 threads: workgroup jb owns trait j and effect l.  Thread i owns the predictors lo + i, lo + i +
// 256, ... of the window, so the only exchange is block-wide sums and maxima in the fixed order of aq_block_sum.  The
// log-sum-exp is two passes (maximum, then sum), once at V_l for alpha and once at the new V_l for the null check.
// aq_k_fm_fit, grid (active tiles, ceil(n / 64)), 256 threads: fit_l[j][i] = sum_s Xs[s][i] (alpha mu)[s][j] on the f64
// matrix pipe for trait tile k and 64 samples, over the tile's items in ascending p0.  Wave w owns the traits 16 w ... 16 w +
// 15 (the B operand) and the four tiles of 16 samples (the A operand, straight from Xs: the sample is the contiguous index,
// so one load is four runs of 128 bytes).  Lane (g, l) holds the predictors p0 + 16 g + step, step = 0 ... 15, of an item: 16
// consecutive alpha and mu of its trait's row, multiplied in registers; an entry outside the trait's window is 0.0 by
// selection, never by multiplication, so what the state holds there cannot reach the result.  Step `step` multiplies the
// predictors p0 + step, + 16, + 32, + 48.  The epilogue goes through an LDS transpose and writes, for active traits only,
// fit_l, Rf = r_l - fit_l and the next effect's panel R = Rf + fit_(l+1), 512 contiguous bytes per trait.
// aq_k_fm_iter_end, grid qb, 256 threads: |Rf|^2, |fit_l|^2, ERSS, the ELBO into the trace, the convergence flag, sigma^2, and
// Rf and R re-formed from y for the next iteration.
// aq_k_fm_rows, grid (Wb, L), 256 threads: the rows (snp, trait, effect, alpha, mu, mu2) with V_l > 0 and alpha >= thr_t from
// the stored state; slots from one 64-bit integer counter that keeps counting beyond cap.
// aq_k_fm_purity, grid = the sets, 256 threads: min and mean |corr| over the pairs of a set's members, a wave per pair.
#pragma once
#include "aq_finemap_plan.h"
#include "aq_screen_tile.h"

struct aq_fm_args {
  const double *Xs, *Yc;               // [p1][n]; [q][n]
  const double *d;                     // p1: x_s' x_s (Sxx of aq_k_ms_colstats)
  int n, p1, q, qa, L;
  const int32_t *item_tile, *item_p0, *first_item;   // the work items of aq_cis_plan.h
  const int32_t *lo, *hi, *orig;       // per ordered trait: the window and the trait's own index
  // the batch
  int k0, w0, j0, qb;                  // its first tile, work item and ordered trait; its traits
  const int32_t *act_items, *act_tiles;   // the items and the tiles with an active trait
  double *Z, *A, *M;
  size_t lstride;                      // doubles of A and M per effect: 64 64 Wb
  double *R, *Rf, *fit;
  // per ordered trait j < qa
  int *act;
  const int *P;
  const double *thr;
  double *sig2, *sig2_used, *elbo_prev;
  double *V, *V_used, *lbf, *szam, *sdam2;   // [L][qa]
  int32_t *n_iter, *conv;
  double *trace;                       // [max_iter][q], under the trait's own index
  int it;
  double tol;
  // the rows
  int32_t *row_snp, *row_trait, *row_effect;
  double *row_alpha, *row_mu, *row_mu2;
  long long cap;
  unsigned long long *n_rows;
};

#define AQ_FM_BLOCK (AQ_CIS_TILE * AQ_CIS_TILE)   // doubles of one item's block

// block-wide maximum in the order of aq_block_sum
__device__ __forceinline__ double aq_fm_block_max(double v, double *sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] = sh[t + s] > sh[t] ? sh[t + s] : sh[t];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

template <bool A16>
__global__ __launch_bounds__(256, 2) void aq_k_fm_xtr(const aq_fm_args a) {
  constexpr int T = AQ_CIS_TILE;
  typedef AqMsShape<T> SH;
  __shared__ __attribute__((aligned(16))) double PX[SH::PAN];
  __shared__ __attribute__((aligned(16))) double PT[SH::PAN];
  const AqMsLane ln;
  const int w = a.act_items[blockIdx.x], p0 = a.item_p0[w], c0 = T * (a.item_tile[w] - a.k0);
  aq_ms_acc<T, 1> acc;
  aq_ms_acc_m<T, false, 1> unused_x, unused_xx;
  const double *panel = a.R;
  // one panel, always live (GUARD = NP: nothing tested); its operands are read together with X's, as in aq_k_cis_tile
  aq_ms_tile_loop<T, false, A16, 1, 1, AQ_MS_STEP_PAIRED>(a.Xs, a.n, a.p1, p0, a.qb, c0, 1, [&](int) { return panel; }, PX, PT, acc, unused_x,
                                                          unused_xx);
  double *z = a.Z + (size_t)(w - a.w0) * AQ_FM_BLOCK;
#pragma unroll
  for (int i = 0; i < SH::NI; i++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int tl = ln.wr * SH::WT + 16 * i + ln.g + 4 * reg;
#pragma unroll
      for (int jj = 0; jj < SH::NI; jj++) z[tl * T + ln.wc * SH::WT + 16 * jj + ln.l] = acc[0][i][jj][reg];
    }
}

static __global__ __launch_bounds__(256) void aq_k_fm_ser(const aq_fm_args a, int l) {
  __shared__ double sh[256];
  const int j = a.j0 + (int)blockIdx.x;
  if (!a.act[j]) return;                                   // uniform over the workgroup
  constexpr int T = AQ_CIS_TILE;
  const int kt = j / T, tl = j % T, lo = a.lo[j], hi = a.hi[j];
  const int w_first = a.first_item[kt], tile_lo = a.item_p0[w_first];
  const size_t lq = (size_t)l * (size_t)a.qa + (size_t)j;
  const double s2 = a.sig2[j], V = a.V[lq], pi = 1.0 / (double)a.P[j], dmin = 1e-10 * (double)a.n;
  const double *z = a.Z;
  const auto at = [&](int s) {                             // the pair's place in a block of the batch
    const int rel = s - tile_lo;
    return (size_t)(w_first - a.w0 + rel / T) * AQ_FM_BLOCK + (size_t)(tl * T + rel % T);
  };
  const auto lbf_of = [&](double zs, double ds, double Vv) {
    const double den = s2 + Vv * ds;
    return Vv == 0.0 ? 0.0 : 0.5 * log(s2 / den) + 0.5 * zs * zs * Vv / (s2 * den);
  };
  // log sum_s pi exp(lbf_s) at prior variance Vv in two passes: *mx the largest lbf_s, *sm = sum_s pi exp(lbf_s - mx)
  const auto lse = [&](double Vv, double *mx, double *sm) {
    double m = -__builtin_inf();
    for (int s = lo + (int)threadIdx.x; s < hi; s += 256) {
      const double ds = a.d[s];
      if (ds > dmin) {
        const double v = lbf_of(z[at(s)], ds, Vv);
        m = v > m ? v : m;
      }
    }
    m = aq_fm_block_max(m, sh);
    double t = 0.0;
    for (int s = lo + (int)threadIdx.x; s < hi; s += 256) {
      const double ds = a.d[s];
      if (ds > dmin) t += pi * exp(lbf_of(z[at(s)], ds, Vv) - m);
    }
    *mx = m;
    *sm = aq_block_sum(t, sh);
  };
  double mx, sm;
  lse(V, &mx, &sm);
  double *A = a.A + (size_t)l * a.lstride, *M = a.M + (size_t)l * a.lstride;
  double vn = 0.0, sz = 0.0, sd = 0.0;
  for (int s = lo + (int)threadIdx.x; s < hi; s += 256) {
    const double ds = a.d[s];
    const size_t o = at(s);
    double al = 0.0, mu = 0.0;
    if (ds > dmin) {
      const double zs = z[o];
      al = pi * exp(lbf_of(zs, ds, V) - mx) / sm;
      const double v = 1.0 / (ds / s2 + 1.0 / V);          // V = 0: 1 / inf = 0
      mu = v * zs / s2;
      const double mu2 = v + mu * mu;
      vn += al * mu2;
      sz += zs * al * mu;
      sd += ds * al * mu2;
    }
    A[o] = al;
    M[o] = mu;
  }
  vn = aq_block_sum(vn, sh);
  sz = aq_block_sum(sz, sh);
  sd = aq_block_sum(sd, sh);
  double mx2, sm2;
  lse(vn, &mx2, &sm2);                                     // the null check at the new prior variance
  if (threadIdx.x == 0) {
    a.lbf[lq] = mx + log(sm);
    a.szam[lq] = sz;
    a.sdam2[lq] = sd;
    a.V_used[lq] = V;
    a.V[lq] = mx2 + log(sm2) <= 0.0 ? 0.0 : vn;
  }
}

static __global__ __launch_bounds__(256) void aq_k_fm_fit(const aq_fm_args a, int l) {
  constexpr int T = AQ_CIS_TILE;
  static_assert(AQ_FM_SAMPLE_BLOCK == 64 && T == 64, "four waves x 16 traits, four tiles of 16 samples");
  __shared__ double tr[T][AQ_FM_SAMPLE_BLOCK + 1];
  const int lane = threadIdx.x & 63, w = (int)(threadIdx.x >> 6), g = lane >> 4, ll = lane & 15;
  const int kt = a.act_tiles[blockIdx.x], i0 = AQ_FM_SAMPLE_BLOCK * (int)blockIdx.y;
  const int tl = 16 * w + ll, j = T * kt + tl;             // the lane's trait: the column of its B operand
  int lo = 0, hi = 0;                                      // an empty window for a trait >= qa
  if (j < a.qa) {
    lo = a.lo[j];
    hi = a.hi[j];
  }
  const size_t n = (size_t)a.n;
  aq_ms_d4 acc[4];
#pragma unroll
  for (int sb = 0; sb < 4; sb++) acc[sb] = aq_ms_d4{0.0, 0.0, 0.0, 0.0};
  for (int wi = a.first_item[kt]; wi < a.first_item[kt + 1]; wi++) {
    const int p0 = a.item_p0[wi];
    const size_t off = (size_t)l * a.lstride + (size_t)(wi - a.w0) * AQ_FM_BLOCK + (size_t)(tl * T + 16 * g);   // a multiple of 16 doubles
    const double2 *pa = reinterpret_cast<const double2 *>(a.A + off), *pm = reinterpret_cast<const double2 *>(a.M + off);
    double b[16];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const double2 va = pa[u], vm = pm[u];
      const int s = p0 + 16 * g + 2 * u;
      b[2 * u] = (s >= lo && s < hi) ? va.x * vm.x : 0.0;
      b[2 * u + 1] = (s + 1 >= lo && s + 1 < hi) ? va.y * vm.y : 0.0;
    }
#pragma unroll
    for (int step = 0; step < 16; step++) {
      const int s = p0 + 16 * g + step;
      const double *xr = a.Xs + (size_t)s * n;             // read only where s < p1
#pragma unroll
      for (int sb = 0; sb < 4; sb++) {
        const int i = i0 + 16 * sb + ll;
        const double x = (s < a.p1 && i < a.n) ? xr[i] : 0.0;
        acc[sb] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, b[step], acc[sb], 0, 0, 0);
      }
    }
  }
  // the accumulator has col = the trait (lane & 15) and row = the sample ((lane >> 4) + 4 reg)
#pragma unroll
  for (int sb = 0; sb < 4; sb++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) tr[tl][16 * sb + g + 4 * reg] = acc[sb][reg];
  __syncthreads();
  const int jb0 = T * (kt - a.k0);
  for (int idx = threadIdx.x; idx < T * AQ_FM_SAMPLE_BLOCK; idx += 256) {
    const int t = idx / AQ_FM_SAMPLE_BLOCK, ii = idx % AQ_FM_SAMPLE_BLOCK, i = i0 + ii, jt = T * kt + t;
    if (jt < a.qa && i < a.n && a.act[jt]) {
      const size_t o = (size_t)(jb0 + t) * n + (size_t)i;
      const size_t fl = (size_t)l * (size_t)a.qb * n;
      const double f = tr[t][ii];
      const double rf = a.R[o] - f;
      a.fit[fl + o] = f;
      a.Rf[o] = rf;
      a.R[o] = l + 1 < a.L ? rf + a.fit[fl + (size_t)a.qb * n + o] : rf;
    }
  }
}

static __global__ __launch_bounds__(256) void aq_k_fm_iter_end(const aq_fm_args a) {
  __shared__ double sh[256];
  const int jb = blockIdx.x, j = a.j0 + jb;
  if (!a.act[j]) return;                                   // uniform over the workgroup
  const size_t n = (size_t)a.n, qbn = (size_t)a.qb * n;
  const double s2 = a.sig2[j], prev = a.elbo_prev[j];
  const int t = a.orig[j];
  double *rf = a.Rf + (size_t)jb * n, *r = a.R + (size_t)jb * n;
  const double *f0 = a.fit + (size_t)jb * n;
  double s = 0.0;
  for (int i = threadIdx.x; i < a.n; i += 256) s += rf[i] * rf[i];
  double erss = aq_block_sum(s, sh), kl = 0.0;
  for (int l = 0; l < a.L; l++) {
    const double *f = f0 + (size_t)l * qbn;
    s = 0.0;
    for (int i = threadIdx.x; i < a.n; i += 256) s += f[i] * f[i];
    const double f2 = aq_block_sum(s, sh);
    const size_t lq = (size_t)l * (size_t)a.qa + (size_t)j;
    erss += a.sdam2[lq] - f2;
    kl += -a.lbf[lq] + (2.0 * a.szam[lq] - a.sdam2[lq]) / (2.0 * s2);
  }
  const double elbo = -0.5 * (double)a.n * log(2.0 * 3.14159265358979323846 * s2) - erss / (2.0 * s2) - kl;
  const bool conv = a.tol > 0.0 && elbo - prev < a.tol;
  if (!conv) {                                             // the next iteration starts from y
    const double *y = a.Yc + (size_t)t * n;
    for (int i = threadIdx.x; i < a.n; i += 256) {
      double v = y[i];
      for (int l = 0; l < a.L; l++) v -= f0[(size_t)l * qbn + i];
      rf[i] = v;
      r[i] = v + f0[i];
    }
  }
  if (threadIdx.x == 0) {                                  // every thread has read s2 and prev before the first barrier
    a.trace[(size_t)a.it * (size_t)a.q + (size_t)t] = elbo;
    a.sig2_used[j] = s2;
    a.elbo_prev[j] = elbo;
    a.n_iter[j] = a.it + 1;
    if (conv) {
      a.conv[j] = 1;
      a.act[j] = 0;
    } else {
      a.sig2[j] = erss / (double)a.n;
    }
  }
}

static __global__ __launch_bounds__(256) void aq_k_fm_rows(const aq_fm_args a) {
  constexpr int T = AQ_CIS_TILE;
  const int w = a.w0 + (int)blockIdx.x, l = blockIdx.y, kt = a.item_tile[w], p0 = a.item_p0[w];
  const size_t base = (size_t)l * a.lstride + (size_t)blockIdx.x * AQ_FM_BLOCK;
  const double dmin = 1e-10 * (double)a.n;
  for (int idx = threadIdx.x; idx < T * T; idx += 256) {
    const int j = T * kt + idx / T, s = p0 + idx % T;
    if (j >= a.qa || a.n_iter[j] < 1 || s < a.lo[j] || s >= a.hi[j]) continue;
    const size_t lq = (size_t)l * (size_t)a.qa + (size_t)j;
    const double ds = a.d[s], al = a.A[base + idx];
    if (!(a.V[lq] > 0.0) || !(ds > dmin) || !(al >= a.thr[j])) continue;
    const unsigned long long slot = atomicAdd(a.n_rows, 1ull);
    if ((long long)slot < a.cap) {
      const double mu = a.M[base + idx], v = 1.0 / (ds / a.sig2_used[j] + 1.0 / a.V_used[lq]);
      a.row_snp[slot] = s;
      a.row_trait[slot] = a.orig[j];
      a.row_effect[slot] = l;
      a.row_alpha[slot] = al;
      a.row_mu[slot] = mu;
      a.row_mu2[slot] = v + mu * mu;
    }
  }
}

// a sum over the wave in a fixed order
__device__ __forceinline__ double aq_fm_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// set b holds the columns set_idx[set_ptr[b]] ... set_idx[set_ptr[b + 1] - 1], 1 ... AQ_FM_PURITY_MAX of them (the host has
// checked).  |corr| of a pair with a constant member counts as 0.
static __global__ __launch_bounds__(256) void aq_k_fm_purity(const double *__restrict__ Xs, int n, const int32_t *__restrict__ set_ptr,
                                                            const int32_t *__restrict__ set_idx, double *__restrict__ min_abs_r,
                                                            double *__restrict__ mean_abs_r) {
  constexpr int MAXP = AQ_FM_PURITY_MAX * (AQ_FM_PURITY_MAX - 1) / 2;
  __shared__ double pr[MAXP];
  __shared__ double mean[AQ_FM_PURITY_MAX], norm[AQ_FM_PURITY_MAX];
  __shared__ double sh[256];
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
  const int32_t *idx = set_idx + set_ptr[blockIdx.x];
  const int m = set_ptr[blockIdx.x + 1] - set_ptr[blockIdx.x], pairs = m * (m - 1) / 2;
  for (int c = wave; c < m; c += 4) {
    const double *x = Xs + (size_t)idx[c] * (size_t)n;
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s += x[i];
    const double mc = aq_fm_wave_sum(s) / (double)n;
    s = 0.0;
    for (int i = lane; i < n; i += 64) s += (x[i] - mc) * (x[i] - mc);
    s = aq_fm_wave_sum(s);
    if (lane == 0) {
      mean[c] = mc;
      norm[c] = s;
    }
  }
  __syncthreads();
  for (int pi = wave; pi < pairs; pi += 4) {
    int c = 0, rem = pi;                                   // pair pi = (c, e), c < e, in the order (0, 1), (0, 2), ...
    while (rem >= m - 1 - c) {
      rem -= m - 1 - c;
      c++;
    }
    const int e = c + 1 + rem;
    const double *x = Xs + (size_t)idx[c] * (size_t)n, *y = Xs + (size_t)idx[e] * (size_t)n;
    const double mc = mean[c], me = mean[e];
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s += (x[i] - mc) * (y[i] - me);
    s = aq_fm_wave_sum(s);
    const double den = norm[c] * norm[e];
    if (lane == 0) pr[pi] = den > 0.0 ? fabs(s) / sqrt(den) : 0.0;
  }
  __syncthreads();
  double mn = __builtin_inf(), sm = 0.0;
  for (int pi = threadIdx.x; pi < pairs; pi += 256) {
    mn = pr[pi] < mn ? pr[pi] : mn;
    sm += pr[pi];
  }
  mn = -aq_fm_block_max(-mn, sh);
  sm = aq_block_sum(sm, sh);
  if (threadIdx.x == 0) {
    min_abs_r[blockIdx.x] = pairs > 0 ? mn : 1.0;
    mean_abs_r[blockIdx.x] = pairs > 0 ? sm / (double)pairs : 1.0;
  }
}
