// aq_postproc.hip -- post-processing of the posterior inclusion probabilities on the device:
//   assign_bFDR        R/summarise_output.R:207-223   Bayesian FDR of every (SNP, trait) pair: sort all p q PPIs in
//                                                     decreasing order (ties in original order), running mean of 1 - PPI
//   hotspot sizes      R/summarise_output.R:98-105, 177-182   rowSums(gam_vb > thres) or rowSums(mat_fdr < thres)
// so that 4-32 GB of PPIs need not travel to the host just to be thresholded.  Sort and scan are hipCUB's
// (rocPRIM radix sort: stable, also in the descending variant; the library is part of ROCm, no hand-written kernel
// beats it for a plain key sort), the rest are three small kernels.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include "aq_internal.h"   // aq_fail, AQ_HIP, AqDev; aq_pair_src, aq_src_pos

template <typename I>
__global__ void aq_k_iota(I *v, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (I)i;
}
__global__ void aq_k_one_minus(const double *__restrict__ x, double *__restrict__ y, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = 1.0 - x[i];
}
// fdr[ind[i]] = cumsum(1 - ppi_ord)[i] / (i + 1)      R/summarise_output.R:213-216
template <typename I>
__global__ void aq_k_bfdr_scatter(const double *__restrict__ cs, const I *__restrict__ ind, double *__restrict__ fdr, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) fdr[ind[i]] = cs[i] / (double)(i + 1);
}

// Descending stable sort of the PPIs with their positions and the running sum of 1 - PPI along that order: the common part
// of assign_bFDR and of the sharded cutoff search below.  Index type: 32 bits below 2^32 entries, 64 bits beyond (the p q
// of C5 on one GPU is 4e9).  Allocates *keys (sorted PPIs), *csum (inclusive running sum of 1 - PPI), *idx (original
// position of each sorted entry).
template <typename I>
static int aq_sort_ppi(const double *d_ppi, size_t n, AqDev<double> *keys, AqDev<double> *csum, AqDev<I> *idx) {
  AqDev<double> tmpd;
  AqDev<I> vin;
  AqDev<char> tmp;
  size_t tb_sort = 0, tb_scan = 0, tb = 0;
  const unsigned grid = (unsigned)((n + 255) / 256);
  AQ_TRY(keys->alloc(n));
  AQ_TRY(csum->alloc(n));
  AQ_TRY(tmpd.alloc(n));
  AQ_TRY(vin.alloc(n));
  AQ_TRY(idx->alloc(n));
  AQ_HIP(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tb_sort, d_ppi, keys->get(), vin.get(), idx->get(), (int64_t)n));
  AQ_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, tb_scan, tmpd.get(), csum->get(), (int64_t)n));
  tb = tb_sort > tb_scan ? tb_sort : tb_scan;
  AQ_TRY(tmp.alloc(tb));
  hipLaunchKernelGGL((aq_k_iota<I>), dim3(grid), dim3(256), 0, 0, vin.get(), n);
  AQ_HIP(hipcub::DeviceRadixSort::SortPairsDescending(tmp.get(), tb, d_ppi, keys->get(), vin.get(), idx->get(), (int64_t)n));   // ind <- order(vec_ppi, decreasing = TRUE)
  hipLaunchKernelGGL(aq_k_one_minus, dim3(grid), dim3(256), 0, 0, keys->get(), tmpd.get(), n);
  AQ_HIP(hipcub::DeviceScan::InclusiveSum(tmp.get(), tb, tmpd.get(), csum->get(), (int64_t)n));                           // cumsum(1 - vec_ppi_ord)
  AQ_HIP(hipGetLastError());
  AQ_HIP(hipDeviceSynchronize());
  return AQ_OK;
}

template <typename I>
static int aq_bfdr_typed(const double *d_ppi, double *d_fdr, size_t n) {
  AqDev<double> keys, csum;
  AqDev<I> idx;
  AQ_TRY(aq_sort_ppi<I>(d_ppi, n, &keys, &csum, &idx));
  hipLaunchKernelGGL((aq_k_bfdr_scatter<I>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, csum.get(), idx.get(), d_fdr, n);
  if (hipDeviceSynchronize() != hipSuccess) return aq_fail(AQ_ERR_DEVICE, "assign_bFDR: scatter failed");
  return AQ_OK;
}

// d_ppi, d_fdr: device vectors of len doubles (as.vector of the p x q matrix); d_fdr may alias nothing.
static bool aq_force_idx64() { const char *e = getenv("AQ_BFDR_IDX64"); return e && e[0] == '1'; }   // test hook: 64-bit positions at any size
int aq_bfdr_device(const double *d_ppi, double *d_fdr, int64_t len) {
  if (len <= 0) return AQ_OK;
  if ((uint64_t)len < (1ull << 32) && !aq_force_idx64()) return aq_bfdr_typed<uint32_t>(d_ppi, d_fdr, (size_t)len);
  return aq_bfdr_typed<uint64_t>(d_ppi, d_fdr, (size_t)len);
}

// ---- Bayesian FDR under trait sharding --------------------------------------------------------------------------------
// assign_bFDR ranks ALL p q PPIs (R/summarise_output.R:207-223).  With the traits spread over ranks, a rank sorts its own
// shard once (aq_shard_sort) and then answers, for a candidate PPI value c, "how many of my entries are >= c / > c and what
// is the sum of 1 - PPI over them" (aq_shard_query: two binary searches on the sorted shard).  Summed over the ranks that
// gives the running mean at the end of c's tie block; the running mean is non-decreasing along the order, so
// {FDR < thres} is a prefix of it and a bisection over c (one 4-double all-reduce per step, driven by the caller) finds it.
struct aq_shard_sorted {
  AqDev<double> keys, csum;
  AqDev<uint32_t> idx32;
  AqDev<uint64_t> idx64;
  size_t n = 0;
};
void aq_shard_free(aq_shard_sorted *s) { delete s; }
int aq_shard_sort(const double *d_ppi, int64_t len, aq_shard_sorted **out) {
  aq_shard_sorted *s = new aq_shard_sorted();
  s->n = (size_t)len;
  int rc = ((uint64_t)len < (1ull << 32) && !aq_force_idx64()) ? aq_sort_ppi<uint32_t>(d_ppi, s->n, &s->keys, &s->csum, &s->idx32)
                                        : aq_sort_ppi<uint64_t>(d_ppi, s->n, &s->keys, &s->csum, &s->idx64);
  if (rc != AQ_OK) { delete s; return rc; }
  *out = s;
  return AQ_OK;
}
// out[0] = #{ppi >= c}, out[1] = sum(1 - ppi : ppi >= c), out[2] = #{ppi > c}, out[3] = sum(1 - ppi : ppi > c),
// out[4] = the largest ppi < c (or -1): the value of the next tie block down
__global__ void aq_k_shard_query(const double *__restrict__ keys, const double *__restrict__ csum, size_t n, double c, double *out) {
  // keys is descending: first position with key < c, first position with key <= c
  size_t lo = 0, hi = n;
  while (lo < hi) { size_t m = lo + (hi - lo) / 2; if (keys[m] >= c) lo = m + 1; else hi = m; }
  const size_t nge = lo;
  lo = 0; hi = nge;
  while (lo < hi) { size_t m = lo + (hi - lo) / 2; if (keys[m] > c) lo = m + 1; else hi = m; }
  const size_t ngt = lo;
  out[0] = (double)nge; out[1] = nge ? csum[nge - 1] : 0.0;
  out[2] = (double)ngt; out[3] = ngt ? csum[ngt - 1] : 0.0;
  out[4] = nge < n ? keys[nge] : -1.0;
}
int aq_shard_query(const aq_shard_sorted *s, double c, double out[5]) {
  AqDev<double> d;
  AQ_TRY(d.alloc(5));
  hipLaunchKernelGGL(aq_k_shard_query, dim3(1), dim3(1), 0, 0, s->keys.get(), s->csum.get(), s->n, c, d.get());
  AQ_HIP(hipMemcpy(out, d.get(), 5 * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}
// rs[j] += 1 for every entry of the first `upto` sorted positions (column-major position -> row = position % p), and for the
// `take` entries of the tie block [t0, t1) that come first in the original order (the sort is stable: block order = index order)
template <typename I>
__global__ void aq_k_shard_rows(const I *__restrict__ idx, size_t upto, size_t t0, size_t take, int p, unsigned long long *rs) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < upto) atomicAdd(&rs[(size_t)idx[i] % (size_t)p], 1ull);
  else if (i - upto < take) atomicAdd(&rs[(size_t)idx[t0 + (i - upto)] % (size_t)p], 1ull);
}
int aq_shard_rows(const aq_shard_sorted *s, int64_t upto, int64_t t0, int64_t take, int p, int64_t *rs_host) {
  AqDev<unsigned long long> d;
  AQ_TRY(d.alloc_zeroed((size_t)p));
  const size_t tot = (size_t)upto + (size_t)take;
  if (tot > 0) {
    const unsigned grid = (unsigned)((tot + 255) / 256);
    if (s->idx32.get()) hipLaunchKernelGGL((aq_k_shard_rows<uint32_t>), dim3(grid), dim3(256), 0, 0, s->idx32.get(), (size_t)upto, (size_t)t0, (size_t)take, p, d.get());
    else hipLaunchKernelGGL((aq_k_shard_rows<uint64_t>), dim3(grid), dim3(256), 0, 0, s->idx64.get(), (size_t)upto, (size_t)t0, (size_t)take, p, d.get());
  }
  AQ_HIP(hipMemcpy(rs_host, d.get(), (size_t)p * sizeof(int64_t), hipMemcpyDeviceToHost));
  return AQ_OK;
}

// rs[j] = #{k : m[j,k] > thres} (lt == 0) or #{k : m[j,k] < thres} (lt == 1); m is p x q column-major
__global__ void aq_k_row_count(const double *__restrict__ m, int64_t *__restrict__ rs, int p, int q, double thres, int lt) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p) return;
  int64_t c = 0;
  for (int k = 0; k < q; k++) {
    double v = m[(size_t)j + (size_t)p * k];
    c += lt ? (v < thres) : (v > thres);
  }
  rs[j] = c;
}
int aq_row_count_device(const double *d_m, int64_t *d_rs, int p, int q, double thres, int lt) {
  hipLaunchKernelGGL(aq_k_row_count, dim3((p + 255) / 256), dim3(256), 0, 0, d_m, d_rs, p, q, thres, lt);
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

// ---- sparse table of associations --------------------------------------------------------------------------------------
// What summary.atlasqtl / plot.atlasqtl do with gam_vb is threshold it (R/summarise_output.R:99-106): gam_vb > thres, or
// assign_bFDR(gam_vb) < thres.  A few thousand to a few million pairs survive out of 5e8 ... 4e9, so the table
//     (snp, trait, ppi, beta = gam_vb mu_beta_vb, fdr),   rows in the order of order(as.vector(gam_vb), decreasing = TRUE)
// is built here and the p x q matrices stay on the device.  In both modes the selected set is a prefix of that order (PPI
// mode: a tie block is in or out as a whole; FDR mode: the running mean of 1 - PPI never decreases along it), so the FDR of
// a row is cumsum(1 - ppi) / (1:N) along the table itself.
//   selection   two passes over the storage, one wave per AQ_SEL_ITEMS consecutive elements: count (ballot + popcount) ->
//               exclusive scan of the wave counts -> write (key, value) at base + rank inside the ballot.  Order-preserving.
//   PPI mode    reads the PPIs where they are -- the trait-tiled gam of a handle [(tile p_pad + j) 16 + k % 16], or a column-
//               major matrix -- and sorts only the selected rows: by position (tiled storage is not in position order), then
//               stably by decreasing PPI.  Scratch: 16 B per wave + 32 B per selected row + the sort's.  Nothing of size p q.
//   FDR mode    aq_sort_ppi as assign_bFDR, then the same selection over the sorted order with the flag
//               csum[i] / (i + 1) < thres: exactly the entries aq_bfdr_device would give an FDR below thres.
#define AQ_SEL_ITEMS 2048   // elements per wave: 32 coalesced reads of 64 doubles

__device__ inline double aq_src_beta(const aq_pair_src &s, uint64_t pos, double ppi) {
  if (!s.mul) return 0.0;
  if (!s.tiled) return s.mul[pos];
  const size_t kk = pos / (size_t)s.p, j = pos - kk * (size_t)s.p;
  return ppi * s.mul[((kk >> 4) * (size_t)s.p_pad + j) * 16 + (kk & 15)];      // gam_vb * mu_beta_vb, R/update_vb.R:17
}

struct aq_sel_ppi {     // gam_vb > thres, R/summarise_output.R:104; value = position
  aq_pair_src s;
  double thres;
  __device__ bool operator()(size_t e, double *key, uint64_t *val) const {
    if (!aq_src_pos(s, e, val)) return false;
    *key = s.ppi[e];
    return *key > thres;
  }
};
struct aq_sel_fdr {     // assign_bFDR(gam_vb) < thres, :100-101, along the sorted order; value = sorted position
  const double *keys, *csum;
  double thres;
  __device__ bool operator()(size_t e, double *key, uint64_t *val) const {
    *key = keys[e];
    *val = e;
    return csum[e] / (double)(e + 1) < thres;
  }
};

template <typename F>
__global__ void aq_k_sel_count(F f, size_t n, unsigned long long *cnt) {
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const size_t e0 = wave * AQ_SEL_ITEMS;
  if (e0 >= n) return;
  unsigned long long c = 0;
  for (int it = 0; it < AQ_SEL_ITEMS / 64; it++) {
    const size_t e = e0 + (size_t)it * 64 + lane;
    double k;
    uint64_t v;
    const bool sel = e < n && f(e, &k, &v);
    c += __popcll(__ballot(sel));
  }
  if (lane == 0) cnt[wave] = c;
}
// rows below `limit` only (the FDR table needs no more than the rows that are returned)
template <typename F>
__global__ void aq_k_sel_write(F f, size_t n, const unsigned long long *__restrict__ off, size_t limit,
                               double *__restrict__ okey, uint64_t *__restrict__ oval) {
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const size_t e0 = wave * AQ_SEL_ITEMS;
  if (e0 >= n) return;
  size_t base = off[wave];
  for (int it = 0; it < AQ_SEL_ITEMS / 64 && base < limit; it++) {
    const size_t e = e0 + (size_t)it * 64 + lane;
    double k = 0.0;
    uint64_t v = 0;
    const bool sel = e < n && f(e, &k, &v);
    const unsigned long long b = __ballot(sel);
    const size_t at = base + __popcll(b & ((1ull << lane) - 1ull));
    if (sel && at < limit) { okey[at] = k; oval[at] = v; }
    base += __popcll(b);
  }
}
// table rows from the selected (key, value) pairs.  idx == NULL: value = position, cs[r] the running sum along the table;
// idx != NULL: value = sorted position i, position = idx[i], cs[i] the running sum along the whole order.
template <typename I>
__global__ void aq_k_pairs_gather(aq_pair_src s, const double *__restrict__ key, const uint64_t *__restrict__ val,
                                  const I *__restrict__ idx, const double *__restrict__ cs, size_t m, int32_t *__restrict__ snp,
                                  int32_t *__restrict__ trait, double *__restrict__ beta, double *__restrict__ fdr) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const size_t i = idx ? (size_t)val[r] : r;
  const uint64_t pos = idx ? (uint64_t)idx[i] : val[r];
  snp[r] = (int32_t)(pos % (uint64_t)s.p);
  trait[r] = (int32_t)(pos / (uint64_t)s.p);
  beta[r] = aq_src_beta(s, pos, key[r]);
  fdr[r] = cs[i] / (double)(i + 1);
}

// count -> scan -> *n_sel; then the first min(limit, *n_sel) selected pairs into *okey / *oval (allocated here; left empty when none)
template <typename F>
static int aq_select_compact(F f, size_t n, int64_t limit, int64_t *n_sel, AqDev<double> *okey, AqDev<uint64_t> *oval) {
  const size_t nw = (n + AQ_SEL_ITEMS - 1) / AQ_SEL_ITEMS;
  const unsigned grid = (unsigned)((nw + 3) / 4);
  AqDev<unsigned long long> cnt, off;
  unsigned long long last[2] = {0, 0};
  AqDev<char> tmp;
  size_t tb = 0, m = 0;
  *n_sel = 0;
  AQ_TRY(cnt.alloc(nw));
  AQ_TRY(off.alloc(nw));
  hipLaunchKernelGGL((aq_k_sel_count<F>), dim3(grid), dim3(256), 0, 0, f, n, cnt.get());
  AQ_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt.get(), off.get(), (int64_t)nw));
  AQ_TRY(tmp.alloc(tb));
  AQ_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.get(), tb, cnt.get(), off.get(), (int64_t)nw));
  AQ_HIP(hipMemcpy(&last[0], cnt.get() + (nw - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost));
  AQ_HIP(hipMemcpy(&last[1], off.get() + (nw - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost));
  *n_sel = (int64_t)(last[0] + last[1]);
  m = (size_t)(limit < *n_sel ? limit : *n_sel);
  if (m > 0) {
    AQ_TRY(okey->alloc(m));
    AQ_TRY(oval->alloc(m));
    hipLaunchKernelGGL((aq_k_sel_write<F>), dim3(grid), dim3(256), 0, 0, f, n, off.get(), m, okey->get(), oval->get());
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipDeviceSynchronize());
  }
  return AQ_OK;
}

// rows [0, m) of the table to the host arrays that were asked for (key = the PPIs in table order)
template <typename I>
static int aq_pairs_emit(const aq_pair_src &src, const double *key, const uint64_t *val, const I *idx, const double *cs, size_t m,
                         int32_t *snp, int32_t *trait, double *ppi, double *beta, double *fdr) {
  AqDev<int32_t> d_i;
  AqDev<double> d_d;
  AQ_TRY(d_i.alloc(2 * m));
  AQ_TRY(d_d.alloc(2 * m));
  hipLaunchKernelGGL((aq_k_pairs_gather<I>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, src, key, val, idx, cs, m, d_i.get(),
                     d_i.get() + m, d_d.get(), d_d.get() + m);
  AQ_HIP(hipGetLastError());
  if (snp) AQ_HIP(hipMemcpy(snp, d_i.get(), m * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (trait) AQ_HIP(hipMemcpy(trait, d_i.get() + m, m * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (ppi) AQ_HIP(hipMemcpy(ppi, key, m * sizeof(double), hipMemcpyDeviceToHost));
  if (beta && src.mul) AQ_HIP(hipMemcpy(beta, d_d.get(), m * sizeof(double), hipMemcpyDeviceToHost));
  if (fdr) AQ_HIP(hipMemcpy(fdr, d_d.get() + m, m * sizeof(double), hipMemcpyDeviceToHost));
  AQ_HIP(hipDeviceSynchronize());
  return AQ_OK;
}

static int aq_pairs_ppi(const aq_pair_src &src, double thres, int64_t cap, int32_t *snp, int32_t *trait, double *ppi, double *beta,
                        double *fdr, int64_t *n_pairs) {
  const size_t n_el = src.tiled ? (size_t)((src.q + 15) / 16) * src.p_pad * 16 : (size_t)src.p * src.q;
  AqDev<double> ka, kb;
  AqDev<uint64_t> va, vb;
  AqDev<char> tmp;
  size_t tb = 0, tb2 = 0, m = 0, N = 0;
  int pos_bits = 1;
  aq_sel_ppi f{src, thres};
  // cap = 0 counts only: nothing is written
  AQ_TRY(aq_select_compact(f, n_el, cap > 0 ? INT64_MAX : 0, n_pairs, &ka, &va));
  N = (size_t)*n_pairs;
  m = (size_t)((int64_t)N < cap ? (int64_t)N : cap);
  if (m == 0) return AQ_OK;
  while (pos_bits < 64 && ((uint64_t)src.p * (uint64_t)src.q) >> pos_bits) pos_bits++;
  AQ_TRY(kb.alloc(N));
  AQ_TRY(vb.alloc(N));
  AQ_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, va.get(), vb.get(), ka.get(), kb.get(), (int64_t)N, 0, pos_bits));
  AQ_HIP(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tb2, kb.get(), ka.get(), vb.get(), va.get(), (int64_t)N));
  if (tb2 > tb) tb = tb2;
  AQ_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, tb2, kb.get(), kb.get(), (int64_t)m));
  if (tb2 > tb) tb = tb2;
  AQ_TRY(tmp.alloc(tb));
  if (src.tiled) {   // the tiled storage is not in position order: order(decreasing = TRUE) breaks ties by position
    AQ_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.get(), tb, va.get(), vb.get(), ka.get(), kb.get(), (int64_t)N, 0, pos_bits));
    AQ_HIP(hipcub::DeviceRadixSort::SortPairsDescending(tmp.get(), tb, kb.get(), ka.get(), vb.get(), va.get(), (int64_t)N));
  } else {
    AQ_HIP(hipcub::DeviceRadixSort::SortPairsDescending(tmp.get(), tb, ka.get(), kb.get(), va.get(), vb.get(), (int64_t)N));
    std::swap(ka, kb);
    std::swap(va, vb);
  }
  // (ka, va) = the table order; kb, vb are free: 1 - ppi and its running sum over the rows that are returned
  hipLaunchKernelGGL(aq_k_one_minus, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, ka.get(), kb.get(), m);
  AQ_HIP(hipcub::DeviceScan::InclusiveSum(tmp.get(), tb, kb.get(), (double *)vb.get(), (int64_t)m));
  AQ_HIP(hipGetLastError());
  return aq_pairs_emit<uint64_t>(src, ka.get(), va.get(), nullptr, (const double *)vb.get(), m, snp, trait, ppi, beta, fdr);
}

template <typename I>
static int aq_pairs_fdr(const double *d_cm, const aq_pair_src &src, double thres, int64_t cap, int32_t *snp, int32_t *trait,
                        double *ppi, double *beta, double *fdr, int64_t *n_pairs) {
  AqDev<double> keys, csum, sk;
  AqDev<uint64_t> sv;
  AqDev<I> idx;
  AQ_TRY(aq_sort_ppi<I>(d_cm, (size_t)src.p * src.q, &keys, &csum, &idx));
  aq_sel_fdr f{keys.get(), csum.get(), thres};
  AQ_TRY(aq_select_compact(f, (size_t)src.p * src.q, cap, n_pairs, &sk, &sv));
  if (sk.get()) {
    const size_t m = (size_t)(*n_pairs < cap ? *n_pairs : cap);
    AQ_TRY(aq_pairs_emit<I>(src, sk.get(), sv.get(), idx.get(), csum.get(), m, snp, trait, ppi, beta, fdr));
  }
  return AQ_OK;
}

// src_ppi / src_mul: the storage the table's ppi and beta are read from (tiled != 0: trait-tiled with p_pad rows per tile);
// d_cm: the same PPIs p x q column-major, needed in FDR mode only (the full sort works on as.vector(gam_vb)).
int aq_pairs_device(const double *d_cm, const double *src_ppi, const double *src_mul, int p, int q, int p_pad, int tiled, double thres,
                    int fdr_adjust, int64_t cap, int32_t *snp, int32_t *trait, double *ppi, double *beta, double *fdr,
                    int64_t *n_pairs) {
  aq_pair_src src{src_ppi, src_mul, p, q, p_pad, tiled};
  if (!fdr_adjust) return aq_pairs_ppi(src, thres, cap, snp, trait, ppi, beta, fdr, n_pairs);
  if ((uint64_t)p * (uint64_t)q < (1ull << 32) && !aq_force_idx64())
    return aq_pairs_fdr<uint32_t>(d_cm, src, thres, cap, snp, trait, ppi, beta, fdr, n_pairs);
  return aq_pairs_fdr<uint64_t>(d_cm, src, thres, cap, snp, trait, ppi, beta, fdr, n_pairs);
}

// rows of a sorted shard (aq_shard_rows' arguments): its first `upto` entries, then `take` entries from sorted position t0
template <typename I>
__global__ void aq_k_shard_pairs(aq_pair_src s, const double *__restrict__ keys, const I *__restrict__ idx, size_t upto, size_t t0,
                                 size_t m, int32_t *__restrict__ snp, int32_t *__restrict__ trait, double *__restrict__ ppi,
                                 double *__restrict__ beta) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const size_t i = r < upto ? r : t0 + (r - upto);
  const uint64_t pos = (uint64_t)idx[i];
  snp[r] = (int32_t)(pos % (uint64_t)s.p);
  trait[r] = (int32_t)(pos / (uint64_t)s.p);
  ppi[r] = keys[i];
  beta[r] = aq_src_beta(s, pos, keys[i]);
}
int aq_shard_pairs(const aq_shard_sorted *sh, int64_t upto, int64_t t0, int64_t take, const double *gam_tile, const double *mu_tile,
                   int p, int q, int p_pad, int32_t *snp, int32_t *trait, double *ppi, double *beta) {
  const size_t m = (size_t)upto + (size_t)take;
  AqDev<int32_t> d_i;
  AqDev<double> d_d;
  aq_pair_src src{gam_tile, mu_tile, p, q, p_pad, 1};
  if (m == 0) return AQ_OK;
  AQ_TRY(d_i.alloc(2 * m));
  AQ_TRY(d_d.alloc(2 * m));
  if (sh->idx32.get())
    hipLaunchKernelGGL((aq_k_shard_pairs<uint32_t>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, src, sh->keys.get(), sh->idx32.get(),
                       (size_t)upto, (size_t)t0, m, d_i.get(), d_i.get() + m, d_d.get(), d_d.get() + m);
  else
    hipLaunchKernelGGL((aq_k_shard_pairs<uint64_t>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, src, sh->keys.get(), sh->idx64.get(),
                       (size_t)upto, (size_t)t0, m, d_i.get(), d_i.get() + m, d_d.get(), d_d.get() + m);
  AQ_HIP(hipGetLastError());
  if (snp) AQ_HIP(hipMemcpy(snp, d_i.get(), m * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (trait) AQ_HIP(hipMemcpy(trait, d_i.get() + m, m * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (ppi) AQ_HIP(hipMemcpy(ppi, d_d.get(), m * sizeof(double), hipMemcpyDeviceToHost));
  if (beta) AQ_HIP(hipMemcpy(beta, d_d.get() + m, m * sizeof(double), hipMemcpyDeviceToHost));
  AQ_HIP(hipDeviceSynchronize());
  return AQ_OK;
}
