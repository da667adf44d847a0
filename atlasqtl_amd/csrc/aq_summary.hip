// aq_summary.hip -- order statistics and moments of the p x q posterior values where they lie: the first
// block of summary.atlasqtl, R/summarise_output.R:89-97,
//     summary(as.vector(object$gam_vb)), summary(as.vector(object$beta_vb))     Min. 1st Qu. Median Mean 3rd Qu. Max.
// Quartiles need a few order statistics, not an ordering, so this is a radix SELECT: histogram one AQ_RSEL_BITS-wide digit
// of the order-preserving 64-bit keys among the values that carry a wanted prefix, pick the bin that holds the wanted rank,
// go on with the next digit.  64 / AQ_RSEL_BITS passes over the storage, every one reading it in place -- the trait-tiled
// gam_vb of a handle, gam_vb * mu_beta_vb formed on the fly (R/update_vb.R:17), or a plain array -- and the only scratch is
// the histogram (n_prefix x 2^AQ_RSEL_BITS counts) and one record of partial moments per workgroup.  Histograms of
// disjoint trait shards add, so the sharded select is exact with one small all-reduce per digit (core.py::radix_select_).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "aq_internal.h"   // aq_fail, AQ_HIP, AqDev; aq_pair_src

#define AQS_BLOCK 256
#define AQS_UNROLL 4          // independent loads in flight per thread (8 measured slower)
#define AQS_MAX_GRID 2048     // capped grid, grid-stride beyond it; fixed, so that the partial sums do not depend on the device
#define AQS_NBIN (1 << AQ_RSEL_BITS)
#define AQS_LEADER_ROUNDS 4   // wave-aggregated adds before the lanes that are left add on their own

static_assert(64 % AQ_RSEL_BITS == 0, "AQ_RSEL_BITS must divide 64");
static_assert(AQ_RSEL_MAX_PREFIX * AQS_NBIN * 8 <= 32768, "histogram must fit 32 KB of LDS");

// (aq_key_of_bits, the order-preserving key of a double: aq_internal.h)
static double aq_value_of_key(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}

// the value of storage element e; false for the padding rows / traits of a tiled array
__device__ inline bool aq_rsel_value(const aq_pair_src &s, size_t e, double *v) {
  uint64_t pos;
  if (!aq_src_pos(s, e, &pos)) return false;
  const double g = s.ppi[e];
  *v = s.mul ? g * s.mul[e] : g;                     // beta_vb = gam_vb * mu_beta_vb, R/update_vb.R:17
  return true;
}

struct aq_rsel_pass {
  int n_prefix, shift;
  uint64_t prefix[AQ_RSEL_MAX_PREFIX];               // key >> (shift + AQ_RSEL_BITS) of the wanted values, ascending
};

// lh[bin] += 1 for every lane with bin >= 0.  Most PPIs share their leading digits, and tie blocks share all of them, so
// nearly every lane of a wave wants the same bin: the lanes that agree with a leader's bin are counted by ballot and added
// once (the ballot / popcount idiom of aq_k_sel_count).  After AQS_LEADER_ROUNDS such rounds the digits are spread, and
// the lanes left add on their own.  Called in wave-uniform control flow.
__device__ inline void aq_rsel_add(unsigned long long *lh, int bin, int lane) {
  unsigned long long todo = __ballot(bin >= 0);
  for (int r = 0; r < AQS_LEADER_ROUNDS && todo; r++) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lb = __shfl(bin, leader);
    const unsigned long long same = __ballot(bin == lb);
    if (lane == leader) atomicAdd(&lh[lb], (unsigned long long)__popcll(same));
    if (bin == lb) bin = -1;
    todo &= ~same;
  }
  if (bin >= 0) atomicAdd(&lh[bin], 1ull);
}

// ghist[i][d] += #{values whose key has prefix[i] above bit shift + AQ_RSEL_BITS and digit d at bit shift}; NaN left out
__global__ __launch_bounds__(AQS_BLOCK) void aq_k_rsel_hist(aq_pair_src s, size_t n_el, aq_rsel_pass a, unsigned long long *ghist) {
  extern __shared__ unsigned long long lh[];         // n_prefix x AQS_NBIN
  const int nb = a.n_prefix * AQS_NBIN;
  const int lane = threadIdx.x & 63;
  const bool top = a.shift + AQ_RSEL_BITS >= 64;     // no bits above the digit: every value takes part
  for (int b = threadIdx.x; b < nb; b += AQS_BLOCK) lh[b] = 0;
  __syncthreads();
  const size_t step = (size_t)gridDim.x * AQS_BLOCK * AQS_UNROLL;
  for (size_t base = (size_t)blockIdx.x * AQS_BLOCK * AQS_UNROLL; base < n_el; base += step) {
    double v[AQS_UNROLL];
    bool ok[AQS_UNROLL];
#pragma unroll
    for (int u = 0; u < AQS_UNROLL; u++) {
      const size_t e = base + (size_t)u * AQS_BLOCK + threadIdx.x;
      v[u] = 0.0;
      ok[u] = e < n_el && aq_rsel_value(s, e, &v[u]);
    }
#pragma unroll
    for (int u = 0; u < AQS_UNROLL; u++) {
      int bin = -1;
      if (ok[u] && v[u] == v[u]) {
        const uint64_t key = aq_key_of_bits((uint64_t)__double_as_longlong(v[u]));
        const int digit = (int)((key >> a.shift) & (uint64_t)(AQS_NBIN - 1));
        if (top) {
          bin = digit;
        } else {
          const uint64_t hp = key >> (a.shift + AQ_RSEL_BITS);
          for (int i = 0; i < a.n_prefix; i++)
            if (hp == a.prefix[i]) bin = i * AQS_NBIN + digit;
        }
      }
      aq_rsel_add(lh, bin, lane);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += AQS_BLOCK)
    if (lh[b]) atomicAdd(&ghist[b], lh[b]);          // one global vector atomic per non-empty bin
}

// one workgroup's share of the moments; min / max as keys (the order the select uses)
struct aq_mom_part {
  unsigned long long count, n_nan, kmin, kmax;
  double sum;
};
__global__ __launch_bounds__(AQS_BLOCK) void aq_k_moments(aq_pair_src s, size_t n_el, aq_mom_part *part) {
  __shared__ aq_mom_part w[AQS_BLOCK / 64];
  unsigned long long cnt = 0, nan = 0, kmin = ~0ull, kmax = 0ull;
  double sum[AQS_UNROLL];
#pragma unroll
  for (int u = 0; u < AQS_UNROLL; u++) sum[u] = 0.0;
  const size_t step = (size_t)gridDim.x * AQS_BLOCK * AQS_UNROLL;
  for (size_t base = (size_t)blockIdx.x * AQS_BLOCK * AQS_UNROLL; base < n_el; base += step) {
#pragma unroll
    for (int u = 0; u < AQS_UNROLL; u++) {
      const size_t e = base + (size_t)u * AQS_BLOCK + threadIdx.x;
      double v;
      if (e < n_el && aq_rsel_value(s, e, &v)) {
        if (v == v) {
          const uint64_t key = aq_key_of_bits((uint64_t)__double_as_longlong(v));
          cnt++;
          sum[u] += v;
          kmin = key < kmin ? key : kmin;
          kmax = key > kmax ? key : kmax;
        } else {
          nan++;
        }
      }
    }
  }
  // fixed-order tree: lanes, then the waves in order -- no floating atomics, the same bits on every call
#pragma unroll
  for (int w = 1; w < AQS_UNROLL; w <<= 1)
#pragma unroll
    for (int u = 0; u + w < AQS_UNROLL; u += 2 * w) sum[u] += sum[u + w];
  double t = sum[0];
  for (int off = 32; off > 0; off >>= 1) {
    t += __shfl_down(t, off);
    cnt += __shfl_down(cnt, off);
    nan += __shfl_down(nan, off);
    const unsigned long long a = __shfl_down(kmin, off), b = __shfl_down(kmax, off);
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
  }
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = aq_mom_part{cnt, nan, kmin, kmax, t};
  __syncthreads();
  if (threadIdx.x == 0) {
    aq_mom_part r = w[0];
    for (int i = 1; i < AQS_BLOCK / 64; i++) {
      r.count += w[i].count;
      r.n_nan += w[i].n_nan;
      r.kmin = w[i].kmin < r.kmin ? w[i].kmin : r.kmin;
      r.kmax = w[i].kmax > r.kmax ? w[i].kmax : r.kmax;
      r.sum += w[i].sum;
    }
    part[blockIdx.x] = r;
  }
}
static_assert((AQS_UNROLL & (AQS_UNROLL - 1)) == 0, "aq_k_moments adds its partial sums pairwise");

static unsigned aq_rsel_grid(size_t n_el) {
  const size_t per = (size_t)AQS_BLOCK * AQS_UNROLL, g = (n_el + per - 1) / per;
  return (unsigned)(g < 1 ? 1 : (g > AQS_MAX_GRID ? AQS_MAX_GRID : g));
}
static double aq_pairwise_sum(const aq_mom_part *p, size_t n) {
  if (n == 1) return p[0].sum;
  return aq_pairwise_sum(p, n / 2) + aq_pairwise_sum(p + n / 2, n - n / 2);
}

// count, n_nan, min, max, sum of the values of src (n_el storage elements), synchronous.  count == 0: min = +Inf, max = -Inf.
int aq_moments_device(const aq_pair_src &src, size_t n_el, aq_moments *out) {
  const unsigned grid = aq_rsel_grid(n_el);
  AqDev<aq_mom_part> d;
  std::vector<aq_mom_part> h(grid);
  uint64_t kmin = ~0ull, kmax = 0ull;
  AQ_TRY(d.alloc(grid));
  hipLaunchKernelGGL(aq_k_moments, dim3(grid), dim3(AQS_BLOCK), 0, 0, src, n_el, d.get());
  AQ_HIP(hipGetLastError());
  AQ_HIP(hipMemcpy(h.data(), d.get(), grid * sizeof(aq_mom_part), hipMemcpyDeviceToHost));
  out->count = out->n_nan = 0;
  for (unsigned i = 0; i < grid; i++) {
    out->count += (int64_t)h[i].count;
    out->n_nan += (int64_t)h[i].n_nan;
    kmin = h[i].kmin < kmin ? h[i].kmin : kmin;
    kmax = h[i].kmax > kmax ? h[i].kmax : kmax;
  }
  out->sum = aq_pairwise_sum(h.data(), grid);        // the workgroups' sums in a fixed pairwise order
  out->min = out->count ? aq_value_of_key(kmin) : HUGE_VAL;
  out->max = out->count ? aq_value_of_key(kmax) : -HUGE_VAL;
  return AQ_OK;
}

// one pass into d_hist (n_prefix x AQS_NBIN, device), copied to hist (host); synchronous
static int aq_rsel_hist_run(const aq_pair_src &src, size_t n_el, const aq_rsel_pass &a, unsigned long long *d_hist, int64_t *hist) {
  const size_t bytes = (size_t)a.n_prefix * AQS_NBIN * sizeof(unsigned long long);
  AQ_HIP(hipMemsetAsync(d_hist, 0, bytes, 0));
  hipLaunchKernelGGL(aq_k_rsel_hist, dim3(aq_rsel_grid(n_el)), dim3(AQS_BLOCK), bytes, 0, src, n_el, a, d_hist);
  AQ_HIP(hipGetLastError());
  AQ_HIP(hipMemcpy(hist, d_hist, bytes, hipMemcpyDeviceToHost));
  return AQ_OK;
}

// prefix: n_prefix ascending values of key >> (shift + AQ_RSEL_BITS); the caller has checked the arguments
int aq_rsel_hist_device(const aq_pair_src &src, size_t n_el, int n_prefix, const uint64_t *prefix, int shift, int64_t *hist) {
  AqDev<unsigned long long> d_hist;
  aq_rsel_pass a;
  memset(&a, 0, sizeof(a));
  a.n_prefix = n_prefix;
  a.shift = shift;
  if (shift + AQ_RSEL_BITS < 64)
    for (int i = 0; i < n_prefix; i++) a.prefix[i] = prefix[i];
  AQ_TRY(d_hist.alloc((size_t)n_prefix * AQS_NBIN));
  return aq_rsel_hist_run(src, n_el, a, d_hist.get(), hist);
}

// out[i] = the ranks[i]-th smallest value (0-based, ranks ascending); *mom the moments.  The digit loop: per wanted rank
// the key prefix found so far and the rank that is left inside it; ranks ascend, so do their prefixes, and equal ones are
// neighbours.
int aq_order_stats_device(const aq_pair_src &src, size_t n_el, int n_ranks, const int64_t *ranks, double *out, aq_moments *mom,
                          const char *who) {
  AqDev<unsigned long long> d_hist;
  std::vector<int64_t> hist((size_t)AQ_RSEL_MAX_PREFIX * AQS_NBIN);
  uint64_t pre[AQ_RSEL_MAX_PREFIX];
  int64_t rem[AQ_RSEL_MAX_PREFIX];
  int slot[AQ_RSEL_MAX_PREFIX];
  aq_moments m;
  AQ_TRY(aq_moments_device(src, n_el, &m));
  if (mom) *mom = m;
  for (int i = 0; i < n_ranks; i++) {
    if (ranks[i] >= m.count)
      return aq_fail(AQ_ERR_ARG, std::string(who) + ": rank " + std::to_string(ranks[i]) + " is not below the number of values (" +
                                         std::to_string(m.count) + ")");
    pre[i] = 0;
    rem[i] = ranks[i];
  }
  AQ_TRY(d_hist.alloc(hist.size()));
  for (int shift = 64 - AQ_RSEL_BITS; shift >= 0; shift -= AQ_RSEL_BITS) {
    aq_rsel_pass a;
    memset(&a, 0, sizeof(a));
    a.shift = shift;
    for (int i = 0; i < n_ranks; i++) {
      if (i == 0 || (shift + AQ_RSEL_BITS < 64 && pre[i] != pre[i - 1])) a.prefix[a.n_prefix++] = pre[i];
      slot[i] = a.n_prefix - 1;
    }
    AQ_TRY(aq_rsel_hist_run(src, n_el, a, d_hist.get(), hist.data()));
    for (int i = 0; i < n_ranks; i++) {
      const int64_t *row = hist.data() + (size_t)slot[i] * AQS_NBIN;
      int64_t below = 0;
      int d = 0;
      while (d < AQS_NBIN && below + row[d] <= rem[i]) below += row[d++];
      if (d == AQS_NBIN) return aq_fail(AQ_ERR_DEVICE, std::string(who) + ": histogram holds fewer values than the moments pass counted");
      rem[i] -= below;
      pre[i] = (pre[i] << AQ_RSEL_BITS) | (uint64_t)d;
    }
  }
  for (int i = 0; i < n_ranks; i++) out[i] = aq_value_of_key(pre[i]);
  return AQ_OK;
}
