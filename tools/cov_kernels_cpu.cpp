// cov_kernels_cpu.cpp -- runs the two kernels of atlasqtl_amd/csrc/aq_cov_kernels.h on the CPU, one workgroup at a time: 256
// host threads per workgroup, a barrier for __syncthreads and a per-wave barrier pair for each shuffle.  It checks the
// kernels' indexing, barrier placement and arithmetic where no GPU is at hand (tools/cov_kernels_cpu.py builds and drives
// it); it says nothing about speed.  aq_xval and aq_block_sum come from aq_prep_dev.h, which the header includes: the macros and
// threadIdx / __syncthreads below are what that header needs on the CPU.
#include <barrier>
#include <thread>
#include <vector>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <cstddef>
struct Idx { int x; };
static thread_local Idx threadIdx, blockIdx;
static std::barrier<> *g_block_bar;
static std::barrier<> *g_wave_bar[4];
static double g_slot[256];
static void __syncthreads() { g_block_bar->arrive_and_wait(); }
static double __shfl_xor(double v, int o, int) {
  const int t = threadIdx.x, w = t >> 6;
  g_slot[t] = v;
  g_wave_bar[w]->arrive_and_wait();
  const double r = g_slot[t ^ o];
  g_wave_bar[w]->arrive_and_wait();
  return r;
}
static double __longlong_as_double(long long b) { double d; memcpy(&d, &b, 8); return d; }
using std::min;
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
double lds[16384];
#include "aq_cov_kernels_host.h"   // the header with its extern __shared__ line rewritten (cov_kernels_cpu.py)

template <typename F> static void run_block(int b, F f) {
  std::barrier<> bb(256), w0(64), w1(64), w2(64), w3(64);
  g_block_bar = &bb; g_wave_bar[0] = &w0; g_wave_bar[1] = &w1; g_wave_bar[2] = &w2; g_wave_bar[3] = &w3;
  std::vector<std::thread> th;
  for (int t = 0; t < 256; t++) th.emplace_back([=, &bb] { threadIdx.x = t; blockIdx.x = b; f(); bb.arrive_and_drop(); g_wave_bar[t >> 6]->arrive_and_drop(); });
  for (auto &x : th) x.join();
}
extern "C" void run_x_f64(const double *X, int n, int p, int D, const double *Qt, double *Xr, uint8_t *ab, double *r2) {
  for (int j = 0; j < p; j++) run_block(j, [=] { aq_k_cov_residualise<double>(X, n, D, Qt, Xr, ab, r2); });
}
extern "C" void run_x_i8(const int8_t *X, int n, int p, int D, const double *Qt, double *Xr, uint8_t *ab, double *r2) {
  for (int j = 0; j < p; j++) run_block(j, [=] { aq_k_cov_residualise<int8_t>(X, n, D, Qt, Xr, ab, r2); });
}
extern "C" void run_y(const double *Y, int n, int q, int D, const double *Qt, double *Yc, int *nobs, int *flag) {
  for (int k = 0; k < q; k++) run_block(k, [=] { aq_k_cov_residualise_y(Y, n, D, Qt, Yc, nobs, flag); });
}
