// aq_predict.hip -- the fitted model applied to genotypes (include/atlasqtl_hip.h, "Prediction"): Yhat = Xt B with
// B = gam_vb * mu_beta_vb read in place from a handle's trait-tiled state (aq_vb_predict, aq_vb_fitted) or uploaded into that
// layout from a dense result (aq_predict), on the f64 matrix pipe (aq_predict_kernels.h, planned by aq_predict_plan.h).
// aq_vb_predict_time times the kernels alone, aq_predict_plan_query runs the planner on the host.  The kernels are plain HIP
// that issues no hand-written load: the ISA proof of the look-ahead sweep units has no operand stream to follow in them; the
// unit's listing goes through the checker in the link step all the same.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdint.h>
#include <string>
#include <vector>
#include "aq_vb.h"                 // aq_vb; aq_internal.h: aq_fail, AQ_HIP, aq_need_device, aq_need_acc_layout, AqDev, aq_tile_from_colmajor
#include "aq_prep.h"               // aq_time_launches
#include "aq_predict_kernels.h"    // aq_k_predict_pack, aq_k_predict_partial, aq_k_predict_reduce; aq_predict_make_plan

// the splits that AQ_PREDICT_SPLITS (test hook) forces whatever p and the CU count say; 0: the variable is not set
static int aq_predict_forced_splits(const char *who, int *force) {
  *force = 0;
  if (const char *e = getenv("AQ_PREDICT_SPLITS")) {
    *force = atoi(e);
    if (*force < 1 || *force > AQ_PREDICT_MAX_SPLITS)
      return aq_fail(AQ_ERR_ARG, std::string(who) + ": AQ_PREDICT_SPLITS must lie in [1, " + std::to_string(AQ_PREDICT_MAX_SPLITS) + "]");
  }
  return AQ_OK;
}

extern "C" int aq_predict_plan_query(int32_t n_new, int32_t p, int32_t q, int32_t ncu, aq_predict_plan *out) {
  if (!out) return aq_fail(AQ_ERR_ARG, "aq_predict_plan_query: NULL argument");
  *out = aq_predict_plan{};
  int force = 0;
  AQ_TRY(aq_predict_forced_splits("aq_predict_plan_query", &force));
  std::string err;
  const int rc = aq_predict_make_plan(n_new, p, q, ncu, force, "aq_predict_plan_query", out, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

// B where it lies: gam (times mu, unless it is NULL) in the trait-tiled layout [>= ceil(q / 16)][p_pad][16]
struct AqPredictB { const double *gam, *mu; int p, q; };
// the rows to predict for: n x p column-major with leading dimension n, fp64 (x) or int8 (x8), on the host or on the device
struct AqPredictX { const double *x; const int8_t *x8; int n; bool on_device; };

// the checks that need no device; `who`: the entry that reports the error
static int aq_predict_args(const char *who, bool have_b, int p, int q, const AqPredictX &X, const double *center, const double *scale,
                           const double *Yhat_out) {
  const std::string w(who);
  if (!have_b) return aq_fail(AQ_ERR_ARG, w + ": NULL handle or beta_vb");
  if (!X.x && !X.x8) return aq_fail(AQ_ERR_ARG, w + ": NULL matrix (X_new and X_new_i8)");
  if (!Yhat_out) return aq_fail(AQ_ERR_ARG, w + ": NULL output");
  if (p < 1 || q < 1) return aq_fail(AQ_ERR_ARG, w + ": p >= 1 and q >= 1 required");
  if (X.n < 1 || X.n > AQ_N_MAX)
    return aq_fail(AQ_ERR_ARG, w + ": n_new must lie in [1, " + std::to_string(AQ_N_MAX) + "] (AQ_N_MAX) per call, " + std::to_string(X.n) + " given");
  if ((center == nullptr) != (scale == nullptr)) return aq_fail(AQ_ERR_ARG, w + ": center and scale must both be given or both be NULL");
  if (scale)
    for (int j = 0; j < p; j++)
      if (!(scale[j] > 0.0) || !std::isfinite(scale[j]) || !std::isfinite(center[j]))
        return aq_fail(AQ_ERR_ARG, w + ": center must be finite and scale finite and positive (predictor " + std::to_string(j + 1) + ")");
  return AQ_OK;
}

// the plan on the current device: its CU count -- or the one that AQ_NCU gives, the hook that overrides it for the sweep's
// plan as well (tests: a small shape then reaches two trait tiles per workgroup) --, and the splits that AQ_PREDICT_SPLITS forces
static int aq_predict_plan_for(int device, int n, int p, int q, const char *who, aq_predict_plan *pl) {
  hipDeviceProp_t prop;
  AQ_HIP(hipGetDeviceProperties(&prop, device));
  int ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (const char *e = getenv("AQ_NCU"))
    if (atoi(e) > 0) ncu = atoi(e);
  int force = 0;
  AQ_TRY(aq_predict_forced_splits(who, &force));
  std::string err;
  const int rc = aq_predict_make_plan(n, p, q, ncu, force, who, pl, &err);
  return rc == AQ_OK ? AQ_OK : aq_fail(rc, err);
}

// the device buffers of one application: the panels of Xt, the partial tiles, Yhat, and the standardisation
struct AqPredictBuf {
  AqDev<double> Xp, scratch, Y, center, inv_scale;
  int alloc(const aq_predict_plan &pl, int n, int q) {
    AQ_TRY(Xp.alloc((size_t)pl.panel_bytes / sizeof(double)));
    AQ_TRY(scratch.alloc((size_t)pl.scratch_bytes / sizeof(double)));
    AQ_TRY(Y.alloc((size_t)n * q));
    return AQ_OK;
  }
  // center and 1 / scale on the device (nothing when both are NULL: the pre-pass then copies)
  int standardisation(const double *c, const double *s, int p) {
    if (!c) return AQ_OK;
    std::vector<double> inv((size_t)p);
    for (int j = 0; j < p; j++) inv[j] = 1.0 / s[j];
    AQ_TRY(center.alloc((size_t)p));
    AQ_TRY(inv_scale.alloc((size_t)p));
    AQ_HIP(hipMemcpy(center.get(), c, (size_t)p * sizeof(double), hipMemcpyHostToDevice));
    AQ_HIP(hipMemcpy(inv_scale.get(), inv.data(), (size_t)p * sizeof(double), hipMemcpyHostToDevice));
    return AQ_OK;
  }
};

template <int NS, int TT>
static void aq_predict_launch_partial(const aq_predict_plan &pl, const AqPredictB &B, const double *Xp, double *scratch) {
  const dim3 grid((unsigned)pl.sample_blocks, (unsigned)pl.trait_groups, (unsigned)pl.splits);
  const long long p_pad = aq_predict_p_pad(B.p);
  const int tiles_q = (B.q + 15) / 16;
  if (B.mu)
    hipLaunchKernelGGL((aq_k_predict_partial<NS, TT, true>), grid, dim3(256), 0, 0, Xp, B.gam, B.mu, B.p, B.q, p_pad, pl.n_pad, tiles_q,
                       pl.chunks_per_split, scratch);
  else
    hipLaunchKernelGGL((aq_k_predict_partial<NS, TT, false>), grid, dim3(256), 0, 0, Xp, B.gam, B.mu, B.p, B.q, p_pad, pl.n_pad, tiles_q,
                       pl.chunks_per_split, scratch);
}

// the pre-pass from the device matrix dX / dX8 (n x p column-major) and the two kernels: b.Y = Xt B (n x q).  Asynchronous.
static int aq_predict_launch(const aq_predict_plan &pl, const AqPredictB &B, const double *dX, const int8_t *dX8, int n, AqPredictBuf &b) {
  // the pre-pass, one workgroup row per sample tile: as many tiles per launch as keep a launch below 2^30 threads
  const long long p_pad = aq_predict_p_pad(B.p);
  const int tiles_n = pl.n_pad / 16;
  const int per_launch = (int)std::max(1ll, std::min(65535ll, (1ll << 30) / (16 * p_pad)));
  for (int it0 = 0; it0 < tiles_n; it0 += per_launch) {
    const dim3 pgrid((unsigned)(p_pad / 16), (unsigned)std::min(per_launch, tiles_n - it0));
    if (dX)
      hipLaunchKernelGGL(aq_k_predict_pack<double>, pgrid, dim3(256), 0, 0, dX, (long long)n, n, B.p, p_pad, b.center.get(), b.inv_scale.get(), it0,
                         b.Xp.get());
    else
      hipLaunchKernelGGL(aq_k_predict_pack<int8_t>, pgrid, dim3(256), 0, 0, dX8, (long long)n, n, B.p, p_pad, b.center.get(), b.inv_scale.get(), it0,
                         b.Xp.get());
  }
  const int ns = pl.sample_tiles / 4;
  auto launch = pl.trait_tiles == 2 ? (ns == 4 ? aq_predict_launch_partial<4, 2> : ns == 2 ? aq_predict_launch_partial<2, 2> : aq_predict_launch_partial<1, 2>)
                                    : (ns == 4 ? aq_predict_launch_partial<4, 1> : ns == 2 ? aq_predict_launch_partial<2, 1> : aq_predict_launch_partial<1, 1>);
  launch(pl, B, b.Xp.get(), b.scratch.get());
  const int tiles_q = (B.q + 15) / 16;
  hipLaunchKernelGGL(aq_k_predict_reduce, dim3((unsigned)((pl.n_pad + 63) / 64), (unsigned)tiles_q), dim3(256), 0, 0, b.scratch.get(), pl.splits,
                     tiles_q, pl.n_pad, n, B.q, b.Y.get());
  AQ_HIP(hipGetLastError());
  return AQ_OK;
}

// the whole application on the current device, after the argument checks: plan, buffers, upload, kernels, copy back
static int aq_predict_apply(const char *who, int device, const AqPredictB &B, const AqPredictX &X, const double *center, const double *scale,
                            double *Yhat_out) {
  AQ_TRY(aq_need_acc_layout(who));
  aq_predict_plan pl{};
  AQ_TRY(aq_predict_plan_for(device, X.n, B.p, B.q, who, &pl));
  AqPredictBuf b;
  AQ_TRY(b.alloc(pl, X.n, B.q));
  AQ_TRY(b.standardisation(center, scale, B.p));
  const size_t np = (size_t)X.n * (size_t)B.p;
  AqDev<double> upx;
  AqDev<int8_t> upx8;
  const double *dX = X.on_device ? X.x : nullptr;
  const int8_t *dX8 = nullptr;
  if (!X.on_device && X.x) {
    AQ_TRY(upx.alloc(np));
    AQ_HIP(hipMemcpy(upx.get(), X.x, np * sizeof(double), hipMemcpyHostToDevice));
    dX = upx.get();
  } else if (!X.on_device) {
    AQ_TRY(upx8.alloc(np));
    AQ_HIP(hipMemcpy(upx8.get(), X.x8, np, hipMemcpyHostToDevice));
    dX8 = upx8.get();
  }
  AQ_TRY(aq_predict_launch(pl, B, dX, dX8, X.n, b));
  AQ_HIP(hipMemcpy(Yhat_out, b.Y.get(), (size_t)X.n * (size_t)B.q * sizeof(double), hipMemcpyDeviceToHost));
  return AQ_OK;
}

// results are about to leave the library: wait for the sweeps and poll the bounded-wait flag, as aq_vb_get_result does
static int aq_predict_handle_ready(aq_vb *s) {
  AQ_HIP(hipSetDevice(s->device));
  AQ_HIP(hipDeviceSynchronize());
  return aq_check_chain_error(s);
}

extern "C" int aq_vb_predict(aq_vb_handle s, const double *X_new, const int8_t *X_new_i8, int32_t n_new, const double *center,
                             const double *scale, double *Yhat_out) {
  const AqPredictX X{X_new, X_new ? nullptr : X_new_i8, n_new, false};
  AQ_TRY(aq_predict_args("aq_vb_predict", s != nullptr, s ? s->p : 1, s ? s->q : 1, X, center, scale, Yhat_out));
  AQ_TRY(aq_predict_handle_ready(s));
  return aq_predict_apply("aq_vb_predict", s->device, AqPredictB{s->gam.get(), s->mu.get(), s->p, s->q}, X, center, scale, Yhat_out);
}

extern "C" int aq_vb_fitted(aq_vb_handle s, const double *Xs_device, double *Yhat_out) {
  const AqPredictX X{Xs_device, nullptr, s ? s->n : 1, true};
  AQ_TRY(aq_predict_args("aq_vb_fitted", s != nullptr, s ? s->p : 1, s ? s->q : 1, X, nullptr, nullptr, Yhat_out));
  AQ_TRY(aq_predict_handle_ready(s));
  return aq_predict_apply("aq_vb_fitted", s->device, AqPredictB{s->gam.get(), s->mu.get(), s->p, s->q}, X, nullptr, nullptr, Yhat_out);
}

extern "C" int aq_predict(const double *beta_vb, int32_t p, int32_t q, const double *X_new, const int8_t *X_new_i8, int32_t n_new,
                          const double *center, const double *scale, double *Yhat_out, int32_t device) {
  const AqPredictX X{X_new, X_new ? nullptr : X_new_i8, n_new, false};
  AQ_TRY(aq_predict_args("aq_predict", beta_vb != nullptr, p, q, X, center, scale, Yhat_out));
  AQ_TRY(aq_need_device(device));
  const int tiles_q = (q + 15) / 16;
  const long long p_pad = aq_predict_p_pad(p);
  AqDev<double> tiled;                           // beta_vb in the layout a handle keeps gam_vb in
  AQ_TRY(tiled.alloc((size_t)tiles_q * (size_t)p_pad * 16));
  {
    AqDev<double> stage;
    AQ_TRY(stage.alloc((size_t)p * (size_t)q));
    AQ_HIP(hipMemcpy(stage.get(), beta_vb, (size_t)p * (size_t)q * sizeof(double), hipMemcpyHostToDevice));
    AQ_TRY(aq_tile_from_colmajor(stage.get(), tiled.get(), p, q, (int)p_pad, tiles_q, 0));
    AQ_HIP(hipDeviceSynchronize());              // `stage` is released here
  }
  return aq_predict_apply("aq_predict", device, AqPredictB{tiled.get(), nullptr, p, q}, X, center, scale, Yhat_out);
}

// Timing hook of aq_vb_predict: the pre-pass (int8 zeros, center 0, scale 1) and the two kernels, `reps` times between two
// events, without the copies from and to the host.
extern "C" int aq_vb_predict_time(aq_vb_handle s, int32_t n_new, int32_t reps, double *ms_per_call, aq_predict_plan *plan_out) {
  if (!s || !ms_per_call) return aq_fail(AQ_ERR_ARG, "aq_vb_predict_time: NULL argument");
  if (reps < 1) return aq_fail(AQ_ERR_ARG, "aq_vb_predict_time: reps >= 1 required");
  if (n_new < 1 || n_new > AQ_N_MAX)
    return aq_fail(AQ_ERR_ARG, "aq_vb_predict_time: n_new must lie in [1, " + std::to_string(AQ_N_MAX) + "] (AQ_N_MAX)");
  AQ_TRY(aq_predict_handle_ready(s));
  AQ_TRY(aq_need_acc_layout("aq_vb_predict_time"));
  aq_predict_plan pl{};
  AQ_TRY(aq_predict_plan_for(s->device, n_new, s->p, s->q, "aq_vb_predict_time", &pl));
  if (plan_out) *plan_out = pl;
  AqPredictBuf b;
  AQ_TRY(b.alloc(pl, n_new, s->q));
  {
    const std::vector<double> zero((size_t)s->p, 0.0), one((size_t)s->p, 1.0);
    AQ_TRY(b.standardisation(zero.data(), one.data(), s->p));
  }
  AqDev<int8_t> dX8;
  AQ_TRY(dX8.alloc_zeroed((size_t)n_new * (size_t)s->p));
  const AqPredictB B{s->gam.get(), s->mu.get(), s->p, s->q};
  return aq_time_launches(reps, ms_per_call, [&] { return aq_predict_launch(pl, B, nullptr, dX8.get(), n_new, b); });
}
