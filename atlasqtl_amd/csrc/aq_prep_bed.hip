// aq_prep_bed.hip -- PLINK 1 .bed input of the prepare entries (include/atlasqtl_hip.h, aq_prepare_data_bed): the genotypes
// arrive as the file stores them, 2 bits each; the packed blocks are uploaded (a quarter of the int8 bytes) and one decode pass
// unpacks them into the int8 buffer that the pipeline of aq_prepare.hip then reads, counting the genotypes of every variant on
// the way (aq_prep_genotype_counts).  With missing = "mean" a missing genotype becomes the mean of its variant's observed ones
// and the matrix fp64.  The checks of the .bed arguments are here too.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>
#include "aq_prep.h"   // aq_prep, the prototypes of what aq_prepare.hip calls here; aq_internal.h

#define AQ_BED_NA (-128)   // a missing genotype in the int8 dosage buffer (never a dosage)

// four 2-bit codes (one .bed byte) -> four dosage bytes, the missing code (1) -> AQ_BED_NA
__device__ __forceinline__ uint32_t aq_bed_dosage4(uint32_t b, int count_a2) {
  uint32_t x = b & 0xffu;
  x = (x | (x << 12)) & 0x000f000fu;
  x = (x | (x << 6)) & 0x03030303u;            // code s in byte s
  const uint32_t H = (x >> 1) & 0x01010101u, L = x & 0x01010101u;
  const uint32_t M = L & ~H;                   // missing
  uint32_t d = H + (H & L);                    // A2 dosage: 0 (hom A1), 1 (het), 2 (hom A2)
  if (!count_a2) d = 0x02020202u - d;          // A1 dosage (every byte <= 2: no borrow between bytes)
  return (d & ~(M * 0xffu)) | (M << 7);
}

__device__ __forceinline__ int8_t aq_bed_dosage1(uint32_t code, int count_a2) {
  if (code == 1) return (int8_t)AQ_BED_NA;
  const int a2 = (int)(code >> 1) + (int)(code == 3);
  return (int8_t)(count_a2 ? a2 : 2 - a2);
}

__device__ __forceinline__ int aq_wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Decode without sample selection: one wave per variant, four variants per workgroup.  The dosage column j starts at byte
// j n of G, its packed block at byte j stride of bed: neither is aligned in general.  The column is cut where its OUTPUT is
// 16-byte aligned: a lane takes 16 genotypes = 32 bits of the block, at any bit offset, out of two aligned dwords (the
// buffer is padded so that both exist) and writes one aligned 16-byte vector; the up to 15 genotypes before the first and
// after the last full vector go one per lane.  The four codes are counted on the packed words (popcount), summed over the
// wave and written by one lane.  All offsets are 64-bit.
__global__ __launch_bounds__(256) void aq_k_bed_decode(const uint32_t *__restrict__ bed32, long long stride, int n, int p,
                                                      int count_a2, int8_t *__restrict__ G, int32_t *__restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= p) return;
  const uint8_t *bed8 = (const uint8_t *)bed32;
  const long long out0 = j * (long long)n, in0 = j * stride;
  const int lead = (int)min((long long)n, (16 - (out0 & 15)) & 15);
  const int nvec = (n - lead) >> 4;
  const int tail0 = lead + (nvec << 4);
  int c_het = 0, c_hom2 = 0, c_mis = 0;
  for (int k = lane; k < nvec; k += 64) {
    const int s0 = lead + (k << 4);
    const long long bit = (in0 << 3) + ((long long)s0 << 1);
    const long long di = bit >> 5;
    const int sh = (int)(bit & 31);
    const unsigned long long ww = ((unsigned long long)bed32[di + 1] << 32) | bed32[di];
    const uint32_t w = (uint32_t)(ww >> sh);
    const uint32_t lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
    c_mis += __popc(lo & ~hi);
    c_het += __popc(hi & ~lo);
    c_hom2 += __popc(hi & lo);
    uint4 v;
    v.x = aq_bed_dosage4(w, count_a2);
    v.y = aq_bed_dosage4(w >> 8, count_a2);
    v.z = aq_bed_dosage4(w >> 16, count_a2);
    v.w = aq_bed_dosage4(w >> 24, count_a2);
    *reinterpret_cast<uint4 *>(G + out0 + s0) = v;
  }
  const int nsingle = lead + (n - tail0);       // <= 30
  if (lane < nsingle) {
    const int s = lane < lead ? lane : tail0 + (lane - lead);
    const uint32_t code = (bed8[in0 + (s >> 2)] >> (2 * (s & 3))) & 3u;
    c_mis += (code == 1); c_het += (code == 2); c_hom2 += (code == 3);
    G[out0 + s] = aq_bed_dosage1(code, count_a2);
  }
  c_mis = aq_wave_sum(c_mis); c_het = aq_wave_sum(c_het); c_hom2 = aq_wave_sum(c_hom2);
  if (lane == 0) {
    int32_t *c = counts + 4 * j;
    c[0] = n - c_mis - c_het - c_hom2; c[1] = c_het; c[2] = c_hom2; c[3] = c_mis;
  }
}

// Decode with sample selection: row i of the column is file sample idx[i], gathered bytewise out of the variant's block
__global__ __launch_bounds__(256) void aq_k_bed_gather(const uint8_t *__restrict__ bed8, long long stride, int n, int p,
                                                      const int32_t *__restrict__ idx, int count_a2, int8_t *__restrict__ G,
                                                      int32_t *__restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= p) return;
  const long long out0 = j * (long long)n, in0 = j * stride;
  int c_het = 0, c_hom2 = 0, c_mis = 0;
  for (int i = lane; i < n; i += 64) {
    const int s = idx[i];
    const uint32_t code = (bed8[in0 + (s >> 2)] >> (2 * (s & 3))) & 3u;
    c_mis += (code == 1); c_het += (code == 2); c_hom2 += (code == 3);
    G[out0 + i] = aq_bed_dosage1(code, count_a2);
  }
  c_mis = aq_wave_sum(c_mis); c_het = aq_wave_sum(c_het); c_hom2 = aq_wave_sum(c_hom2);
  if (lane == 0) {
    int32_t *c = counts + 4 * j;
    c[0] = n - c_mis - c_het - c_hom2; c[1] = c_het; c[2] = c_hom2; c[3] = c_mis;
  }
}

// int8 dosages -> fp64 with the variant's own value (fill[j]) in place of a missing genotype
__global__ __launch_bounds__(256) void aq_k_bed_impute(const int8_t *__restrict__ G, int n, const double *__restrict__ fill,
                                                      double *__restrict__ X) {
  const size_t base = (size_t)blockIdx.x * n;
  const double f = fill[blockIdx.x];
  for (int i = threadIdx.x; i < n; i += 256) {
    const int8_t g = G[base + i];
    X[base + i] = g == (int8_t)AQ_BED_NA ? f : (double)g;
  }
}

// the decode pass: packed blocks -> *dG_out (n x p int8, AQ_BED_NA = missing) and h->gcounts
static int aq_bed_decode(aq_prep *h, const aq_prep_bed_input *in, AqDev<int8_t> *dG_out) {
  const int n = h->n, p = h->p;
  const size_t stride = ((size_t)in->n_file + 3) / 4, nbytes = (size_t)p * stride;
  AqDev<uint32_t> dbed;
  AqDev<int32_t> didx, dcnt;
  const unsigned grid = (unsigned)(((long long)p + 3) / 4);
  // two dwords of padding: the aligned pair a lane reads may end one dword past the last block (those bits are shifted out)
  AQ_TRY(dbed.alloc(nbytes / 4 + 3));
  AQ_HIP(hipMemcpy(dbed.get(), in->bed, nbytes, hipMemcpyHostToDevice));
  AQ_TRY(dG_out->alloc((size_t)n * p));
  AQ_TRY(dcnt.alloc((size_t)4 * p));
  if (in->sample_idx) {
    AQ_TRY(didx.alloc((size_t)n));
    AQ_HIP(hipMemcpy(didx.get(), in->sample_idx, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(aq_k_bed_gather, dim3(grid), dim3(256), 0, 0, (const uint8_t *)dbed.get(), (long long)stride, n, p, didx.get(),
                       in->count_a2, dG_out->get(), dcnt.get());
  } else {
    hipLaunchKernelGGL(aq_k_bed_decode, dim3(grid), dim3(256), 0, 0, dbed.get(), (long long)stride, n, p, in->count_a2, dG_out->get(), dcnt.get());
  }
  AQ_HIP(hipGetLastError());
  h->gcounts.resize((size_t)4 * p);
  AQ_HIP(hipMemcpy(h->gcounts.data(), dcnt.get(), h->gcounts.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  return AQ_OK;
}

// the checks of aq_prepare_data_bed's own arguments; every entry that takes a .bed input reports them under that name
int aq_bed_check_args(const aq_prep_bed_input *in) {
  if (in->n > in->n_file)
    return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: n = " + std::to_string(in->n) + " rows asked of a file with n_file = " +
                                       std::to_string(in->n_file) + " samples");
  if (!in->sample_idx && in->n != in->n_file)
    return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: sample_idx is NULL, so n = " + std::to_string(in->n) +
                                       " must equal n_file = " + std::to_string(in->n_file));
  if (in->sample_idx)
    for (int i = 0; i < in->n; i++)
      if (in->sample_idx[i] < 0 || in->sample_idx[i] >= in->n_file)
        return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: sample_idx[" + std::to_string(i) + "] = " +
                                           std::to_string(in->sample_idx[i]) + " is out of range [0, " + std::to_string(in->n_file) + ")");
  if ((in->count_a2 != 0 && in->count_a2 != 1) || (in->missing != 0 && in->missing != 1))
    return aq_fail(AQ_ERR_ARG, "aq_prepare_data_bed: count_a2 and missing must be 0 or 1");
  return AQ_OK;
}

// decode and count; without a missing genotype the dosages stay int8 in *dG, else they are an error or imputed into *dX
int aq_bed_source(aq_prep *h, const aq_prep_bed_input *in, AqDev<int8_t> *dG, AqDev<double> *dX) {
  long long n_mis = 0, p_mis = 0, first_mis = -1;
  AQ_TRY(aq_bed_decode(h, in, dG));
  for (int j = 0; j < in->p; j++) {
    const int m = h->gcounts[4 * (size_t)j + 3];
    if (m > 0) { n_mis += m; p_mis++; if (first_mis < 0) first_mis = j; }
  }
  if (n_mis == 0) return AQ_OK;
  if (!in->missing)
    return aq_fail(AQ_ERR_ARG, "X must be a non-empty a numeric matrix, finite without missing value. " + std::to_string(n_mis) +
                                     " genotype(s) in " + std::to_string(p_mis) + " variant(s) are missing among the " +
                                     std::to_string(in->n) + " samples used; the first such variant has index " +
                                     std::to_string(first_mis) + " (0-based, among the variants given). missing = \"mean\" replaces "
                                     "a missing genotype by the mean of its variant's observed ones.");
  std::vector<double> fill(in->p);
  AqDev<double> dfill;
  for (int j = 0; j < in->p; j++) {   // (n_het + 2 n_hom_counted) / n_obs: one fp64 division of exact integers
    const int32_t *c = &h->gcounts[4 * (size_t)j];
    const int n_obs = c[0] + c[1] + c[2];
    fill[j] = n_obs > 0 ? (double)(c[1] + 2 * (long long)(in->count_a2 ? c[2] : c[0])) / (double)n_obs : 0.0;
  }
  AQ_TRY(dfill.alloc((size_t)in->p));
  AQ_HIP(hipMemcpy(dfill.get(), fill.data(), (size_t)in->p * sizeof(double), hipMemcpyHostToDevice));
  AQ_TRY(dX->alloc((size_t)in->n * in->p));
  hipLaunchKernelGGL(aq_k_bed_impute, dim3(in->p), dim3(256), 0, 0, dG->get(), in->n, dfill.get(), dX->get());
  AQ_HIP(hipGetLastError());
  AQ_HIP(hipDeviceSynchronize());
  dG->reset();
  return AQ_OK;
}

extern "C" int aq_prep_genotype_counts(aq_prep_handle h, int32_t *counts) {
  if (!h || !counts) return aq_fail(AQ_ERR_ARG, "aq_prep_genotype_counts: NULL argument");
  if (h->gcounts.empty())
    return aq_fail(AQ_ERR_ARG, "aq_prep_genotype_counts: the handle was not made by aq_prepare_data_bed");
  std::copy(h->gcounts.begin(), h->gcounts.end(), counts);
  return AQ_OK;
}
