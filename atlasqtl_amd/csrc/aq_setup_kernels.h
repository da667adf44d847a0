// aq_setup_kernels.h -- the kernels that run once per handle, from aq_vb_create: the MFMA operand layouts and Gram blocks of X,
// the initial values drawn on the device, the row panels and the per-trait Gram blocks of the masked kernels.
// Non-template kernels: included by aq_vb_create.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include "aq_special.h"
#include "aq_core_sweep.h"   // aq_mfma, AQ_GK_STRIDE

// ---------------------------------------------------------------- layouts ----
__device__ __forceinline__ int aqv_drow(int dmode, int reg, int g) { return dmode ? (4 * g + reg) : (4 * reg + g); }

// X (n x p, R column-major) -> XA / XU MFMA operand layouts (see aq_core_sweep.h)
__global__ void aq_k_build_x_layouts(const double *__restrict__ X, double2 *__restrict__ XA,
                                     double2 *__restrict__ XU, int n, int p, int nb, int NTT, int dmode) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)nb * NTT * 128;
  if (e >= total) return;
  int lane = (int)(e & 63);
  int h = (int)((e >> 6) & 1);
  size_t bt = e >> 7;
  int T = (int)(bt % NTT);
  int b = (int)(bt / NTT);
  int g = lane >> 4, c15 = lane & 15;
  {
    int snp = 16 * b + c15;
    int s0 = 16 * T + aqv_drow(dmode, 2 * h, g), s1 = 16 * T + aqv_drow(dmode, 2 * h + 1, g);
    double2 v;
    v.x = (snp < p && s0 < n) ? X[(size_t)s0 + (size_t)n * snp] : 0.0;
    v.y = (snp < p && s1 < n) ? X[(size_t)s1 + (size_t)n * snp] : 0.0;
    XA[e] = v;
  }
  {
    int s = 16 * T + c15;
    int j0 = 16 * b + 4 * (2 * h) + g, j1 = 16 * b + 4 * (2 * h + 1) + g;
    double2 v;
    v.x = (s < n && j0 < p) ? X[(size_t)s + (size_t)n * j0] : 0.0;
    v.y = (s < n && j1 < p) ? X[(size_t)s + (size_t)n * j1] : 0.0;
    XU[e] = v;
  }
}

// x' y over n samples with compensated (Kahan) summation: the error stays at a few ulp for any n.  A plain running sum loses about
// sqrt(n) ulp -- 5e-14 relative in the worst of 9000 entries at n = 4000 -- and with missing values the diagonal of these blocks is
// X_norm_sq(j, k), which goes into mu_beta_vb and tau_vb entry by entry (tests/test_gpu_link_range.py, wide-c12-na).  Once per handle.
__device__ __forceinline__ double aq_dot_kahan(const double *__restrict__ x, const double *__restrict__ y, int n) {
  double s = 0.0, c = 0.0;
  for (int r = 0; r < n; r++) {
    const double t = x[r] * y[r] - c;
    const double u = s + t;
    c = (u - s) - t;
    s = u;
  }
  return s;
}

// diagonal Gram blocks G[b] = X_b' X_b and first off-diagonal blocks Gx[b] = X_b' X_{b-1} (16 x 16 each):
// the only parts of cp_X (R/atlasqtl_global_local_core.R:41) the blocked recursion needs
__global__ void aq_k_gram_blocks(const double *__restrict__ X, double *__restrict__ G, double *__restrict__ Gx, int n,
                                 int p) {
  int b = blockIdx.x;
  int i = threadIdx.x >> 4, j = threadIdx.x & 15;
  int ji = 16 * b + i, jj = 16 * b + j;
  {   // cross block with the previous SNP block: Gx[b][i][j] = x_{16b+i}' x_{16(b-1)+j}
    int jp = 16 * (b - 1) + j;
    double sx = 0.0;
    if (b > 0 && ji < p && jp < p) sx = aq_dot_kahan(X + (size_t)n * ji, X + (size_t)n * jp, n);
    Gx[(size_t)b * 256 + threadIdx.x] = sx;
  }
  double s = 0.0;
  if (ji < p && jj < p) {     // (the smaller index first: G stays exactly symmetric)
    const int lo = i <= j ? ji : jj, hi = i <= j ? jj : ji;
    s = aq_dot_kahan(X + (size_t)n * lo, X + (size_t)n * hi, n);
  }
  G[(size_t)b * 256 + threadIdx.x] = s;
}

// ----------------------------------------------- initial values on the device ----
// auto_set_init_ (R/set_hyper_init.R:385-387): gam_vb = pnorm(rnorm(p q, mean = n0, sd = s02 + t02)), mu_beta_vb = rnorm(p q).
// R's Mersenne-Twister stream cannot be reproduced anyway, so the draws come from a counter-based generator
// that any shard can evaluate on its own: Philox4x32-10 (Salmon et al., SC'11) keyed by the seed, counter = (SNP j, global
// trait k, 0, 0); one call yields both normals of the entry (Box-Muller).  the CPU checker under tests/ restates the same stream.
__host__ __device__ inline void aq_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
__host__ __device__ inline void aq_init_pair(uint64_t seed, uint32_t j, uint32_t k_global, double gam_mean, double gam_sd,
                                             double *gam, double *mu) {
  uint32_t c[4] = {j, k_global, 0u, 0u};
  aq_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  // two uniforms in (0, 1) with 53 bits each
  const double u1 = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6) + 0.5) * (1.0 / 9007199254740992.0);
  const double u2 = ((double)(c[2] >> 5) * 67108864.0 + (double)(c[3] >> 6) + 0.5) * (1.0 / 9007199254740992.0);
  const double r = sqrt(-2.0 * log(u1));
  const double z1 = r * cos(6.283185307179586476925286766559 * u2), z2 = r * sin(6.283185307179586476925286766559 * u2);
  *gam = 0.5 * erfc(-(gam_mean + gam_sd * z1) * 0.70710678118654752440084436210485);    // pnorm
  *mu = z2;
}
// gam, mu in the trait-tiled layout [ntile][p_pad][16]; padding entries are 0
__global__ void aq_k_init_generate(double *__restrict__ gam, double *__restrict__ mu, int p, int q, int p_pad, int ntile,
                                   unsigned long long seed, int trait_offset, double gam_mean, double gam_sd) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)ntile * p_pad * 16;
  if (e >= total) return;
  int hk = (int)(e & 15);
  size_t rest = e >> 4;
  int j = (int)(rest % p_pad), tile = (int)(rest / p_pad);
  int k = tile * 16 + hk;
  double g = 0.0, m = 0.0;
  if (j < p && k < q) aq_init_pair(seed, (uint32_t)j, (uint32_t)(trait_offset + k), gam_mean, gam_sd, &g, &m);
  gam[e] = g;
  mu[e] = m;
}

// X_b in row-major panels for the gathers: XR[(b*NR + i)*16 + jj] = x_{i, 16 b + jj} (0 beyond n or p)
__global__ void aq_k_build_xr(const double *__restrict__ X, double *__restrict__ XR, int n, int p, int nb, int NR) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)nb * NR * 16;
  if (e >= total) return;
  int jj = (int)(e & 15);
  size_t rest = e >> 4;
  int i = (int)(rest % NR);
  int b = (int)(rest / NR);
  int j = 16 * b + jj;
  XR[e] = (i < n && j < p) ? X[(size_t)i + (size_t)n * j] : 0.0;
}

// ---- per-trait Gram blocks for the masked form of the look-ahead kernel (AqCoreArgs::GK) -------------------------------------
// For every trait tile and SNP block b, and each of the tile's 16 traits k:
//     diagonal block  X_b' diag(mis_k) X_b     = X_b'X_b     - Xm_k(b)' Xm_k(b)        lower triangle [i (i + 1) / 2 + j][k]
//     cross block     X_b' diag(mis_k) X_{b-1} = X_b'X_{b-1} - Xm_k(b)' Xm_k(b-1)      [i][j][k]
// (Xm_k(b) = the rows of X_b at trait k's missing samples: rank-m_k f64-MFMA corrections from gathered 128-byte row segments,
// as compute_gk above).  They depend on X and on the missingness pattern only, so they are computed ONCE per handle and kept in
// HBM -- 50 KB per (tile, block), 98 GB for a C5 trait shard: what 288 GB are for -- instead of being recomputed by every sweep
// (2 m_k 256 flop per trait and block, a third of the sweep's MFMA work at 5 % missing, and the cross blocks would double it).
// grid = (ceil(nb / bchunk), ntile), 512 threads; wave w handles the jobs (trait, kind) = w, w + 8, ... of each block.
__global__ __launch_bounds__(512) void aq_k_gk_blocks(const double *__restrict__ XR, const double *__restrict__ G,
                                                    const double *__restrict__ Gx, const int *__restrict__ midx,
                                                    const int *__restrict__ mcnt4, double *__restrict__ GK, int nb, int NR, int Mmax,
                                                    int bchunk) {
  extern __shared__ unsigned short aq_gk_lidx[];   // [16][Mmax]
  __shared__ int Lcnt[16];
  const int tile = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, col = lane & 15;
  for (int e = tid; e < 16 * Mmax; e += 512) aq_gk_lidx[e] = (unsigned short)midx[(size_t)tile * 16 * Mmax + e];
  if (tid < 16) Lcnt[tid] = mcnt4[tile * 16 + tid];
  __syncthreads();
  const int b0 = blockIdx.x * bchunk, b1 = min(nb, b0 + bchunk);
  for (int b = b0; b < b1; b++) {
    double *out = GK + ((size_t)tile * nb + b) * AQ_GK_STRIDE;
    const double *xr = XR + (size_t)b * NR * 16 + col;
    const double *xp = XR + (size_t)(b > 0 ? b - 1 : 0) * NR * 16 + col;
    for (int job = w; job < 32; job += 8) {
      const int k = job & 15, cross = job >> 4;
      aq_d4 acc = (aq_d4){0, 0, 0, 0};
      const int n4 = (cross && b == 0) ? 0 : Lcnt[k];
      const unsigned short *ix = aq_gk_lidx + k * Mmax + g;
      for (int t = 0; t < n4; t += 4) {   // lists are padded to whole groups of 16 samples (index n_pad = an all-zero row)
        const int i0 = ix[4 * t], i1 = ix[4 * t + 4], i2 = ix[4 * t + 8], i3 = ix[4 * t + 12];
        const double a0 = xr[(size_t)i0 * 16], a1 = xr[(size_t)i1 * 16], a2 = xr[(size_t)i2 * 16], a3 = xr[(size_t)i3 * 16];
        if (cross) {
          const double c0 = xp[(size_t)i0 * 16], c1 = xp[(size_t)i1 * 16], c2 = xp[(size_t)i2 * 16], c3 = xp[(size_t)i3 * 16];
          acc = aq_mfma(a0, c0, acc); acc = aq_mfma(a1, c1, acc); acc = aq_mfma(a2, c2, acc); acc = aq_mfma(a3, c3, acc);
        } else {
          acc = aq_mfma(a0, a0, acc); acc = aq_mfma(a1, a1, acc); acc = aq_mfma(a2, a2, acc); acc = aq_mfma(a3, a3, acc);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * r + g, j = col;            // D layout: row = 4 reg + (lane >> 4), column = lane & 15
        if (cross) {
          const double base = b > 0 ? Gx[(size_t)b * 256 + i * 16 + j] : 0.0;
          out[AQ_GK_DIAG + (i * 16 + j) * 16 + k] = base - acc[r];
        } else if (i >= j) {
          out[(i * (i + 1) / 2 + j) * 16 + k] = G[(size_t)b * 256 + i * 16 + j] - acc[r];
        }
      }
    }
  }
}

// ---- the diagonal of the per-trait Gram blocks where the subtraction cancels ---------------------------------------------------
// X_norm_sq(j, k) = G_jj - sum over trait k's missing samples of x_ij^2 is the diagonal of the blocks above.  When the missing
// samples carry almost all of x_j' x_j -- a rare variant whose carriers are all missing in trait k: G_jj = n - 1, X_norm_sq(j, k)
// about 1 -- the difference keeps an absolute error of a few ulp of n, 4e-13 of its own size at n = 4000, and that entry's
// sig2_beta_vb, mu_beta_vb and the trait's tau_vb inherit it (tests/test_gpu_regimes.py, mask-n1000-*, mask-wide-c12-*: tau_vb off
// by up to 4e-12 after three sweeps, where the n-space reference holds 6e-15).  Such entries -- less than an eighth of G_jj left
// -- are redone here with both sums carried in double-double (error-free products by FMA, two-sum accumulation), so that the
// difference is exact to the last place.  One thread per (tile, block, SNP, trait); only the few affected threads loop.  Once per handle.
__global__ void aq_k_gk_diag_exact(const double *__restrict__ XR, const double *__restrict__ G, const int *__restrict__ midx,
                                   const int *__restrict__ mcnt4, const int *__restrict__ obs, double *__restrict__ GK, int n, int nb,
                                   int ntile, int NR, int Mmax) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)ntile * nb * 256) return;
  const int k = (int)(e & 15), jj = (int)((e >> 4) & 15);
  const size_t tb = e >> 8;
  const int b = (int)(tb % nb), tile = (int)(tb / nb);
  if (obs && obs[tile * 16 + k]) return;               // summed over the observed samples directly: nothing cancels
  double *dst = GK + ((size_t)tile * nb + b) * AQ_GK_STRIDE + (size_t)(jj * (jj + 1) / 2 + jj) * 16 + k;
  const double gjj = G[(size_t)b * 256 + jj * 17];
  if (!(*dst < 0.125 * gjj)) return;
  const double *x = XR + (size_t)b * NR * 16 + jj;
  double hi[2] = {0.0, 0.0}, lo[2] = {0.0, 0.0};
  const int *ix = midx + ((size_t)tile * 16 + k) * Mmax;
  const int m = 4 * mcnt4[tile * 16 + k];
  for (int pass = 0; pass < 2; pass++) {
    const int cnt = pass == 0 ? n : m;
    for (int t = 0; t < cnt; t++) {
      const double v = x[(size_t)(pass == 0 ? t : ix[t]) * 16];
      const double pr = __dmul_rn(v, v), pe = __fma_rn(v, v, -pr);    // v^2 = pr + pe exactly (_rn: never contracted)
      const double sm = __dadd_rn(hi[pass], pr), bb = __dsub_rn(sm, hi[pass]);
      lo[pass] += __dadd_rn(__dadd_rn(__dsub_rn(hi[pass], __dsub_rn(sm, bb)), __dsub_rn(pr, bb)), pe);
      hi[pass] = sm;
    }
  }
  *dst = (hi[0] - hi[1]) + (lo[0] - lo[1]);
}

// ---- per-trait Gram blocks for the wide sample split (n > 10240): the same blocks as aq_k_gk_blocks, for any missingness ------
// The index lists stay in global memory (int32, [ntile][16][Mmax], padded to groups of 16 with the all-zero row n_pad of XR), and
// each trait uses the shorter of its two lists: obs[k] = 0 -- the missing samples, blocks = G - Xm' Xm as above; obs[k] = 1 -- the
// observed samples, blocks = Xo' Xo directly.  Either way at most n / 2 rows per trait.  Once per handle.
__global__ __launch_bounds__(512) void aq_k_gk_blocks_g(const double *__restrict__ XR, const double *__restrict__ G,
                                                      const double *__restrict__ Gx, const int *__restrict__ midx,
                                                      const int *__restrict__ mcnt4, const int *__restrict__ obs,
                                                      double *__restrict__ GK, int nb, int NR, int Mmax, int bchunk) {
  const int tile = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, col = lane & 15;
  const int b0 = blockIdx.x * bchunk, b1 = min(nb, b0 + bchunk);
  for (int b = b0; b < b1; b++) {
    double *out = GK + ((size_t)tile * nb + b) * AQ_GK_STRIDE;
    const double *xr = XR + (size_t)b * NR * 16 + col;
    const double *xp = XR + (size_t)(b > 0 ? b - 1 : 0) * NR * 16 + col;
    for (int job = w; job < 32; job += 8) {
      const int k = job & 15, cross = job >> 4;
      const bool direct = obs[tile * 16 + k] != 0;
      aq_d4 acc = (aq_d4){0, 0, 0, 0};
      const int n4 = (cross && b == 0) ? 0 : mcnt4[tile * 16 + k];
      const int *ix = midx + ((size_t)tile * 16 + k) * Mmax + g;
      for (int t = 0; t < n4; t += 4) {
        const int i0 = ix[4 * t], i1 = ix[4 * t + 4], i2 = ix[4 * t + 8], i3 = ix[4 * t + 12];
        const double a0 = xr[(size_t)i0 * 16], a1 = xr[(size_t)i1 * 16], a2 = xr[(size_t)i2 * 16], a3 = xr[(size_t)i3 * 16];
        if (cross) {
          const double c0 = xp[(size_t)i0 * 16], c1 = xp[(size_t)i1 * 16], c2 = xp[(size_t)i2 * 16], c3 = xp[(size_t)i3 * 16];
          acc = aq_mfma(a0, c0, acc); acc = aq_mfma(a1, c1, acc); acc = aq_mfma(a2, c2, acc); acc = aq_mfma(a3, c3, acc);
        } else {
          acc = aq_mfma(a0, a0, acc); acc = aq_mfma(a1, a1, acc); acc = aq_mfma(a2, a2, acc); acc = aq_mfma(a3, a3, acc);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * r + g, j = col;            // D layout: row = 4 reg + (lane >> 4), column = lane & 15
        if (cross) {
          const double base = (b > 0 && !direct) ? Gx[(size_t)b * 256 + i * 16 + j] : 0.0;
          out[AQ_GK_DIAG + (i * 16 + j) * 16 + k] = direct ? (b > 0 ? acc[r] : 0.0) : base - acc[r];
        } else if (i >= j) {
          out[(i * (i + 1) / 2 + j) * 16 + k] = direct ? acc[r] : G[(size_t)b * 256 + i * 16 + j] - acc[r];
        }
      }
    }
  }
}
