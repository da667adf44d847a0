// aq_internal.h -- the one internal interface of libatlasqtl_hip.so: error plumbing, the owner of device memory and the
// prototype of every function that one translation unit calls in another.  Every unit that defines or calls one of them
// includes this header, so a definition that differs from its declaration is a compile error.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/atlasqtl_hip.h"
#include "aq_pair_src.h"

// ------------------------------------------------------------------ errors ----
// sets this thread's aq_last_error() and returns code (aq_ops.hip)
int aq_fail(int code, const std::string &msg);
#define AQ_HIP(call)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (call);                                                                            \
    if (e_ != hipSuccess)                                                                              \
      return aq_fail(AQ_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + \
                                        std::to_string(__LINE__) + ")");                               \
  } while (0)
#define AQ_TRY(x)            \
  do {                       \
    int rc_ = (x);           \
    if (rc_ != AQ_OK) return rc_; \
  } while (0)

// a HIP device is visible, `device` names one, and it is the current one (aq_ops.hip)
int aq_need_device(int device);

// ----------------------------------------------------------- device memory ----
// The owner of a device allocation: move-only, frees in its destructor.  Buffers handed in from outside (the caller's
// all-reduce payloads, a device-resident X) stay raw pointers.
extern std::atomic<int64_t> aq_live_device_bytes;   // held by AqDev objects in this process (aq_ops.hip)

template <typename T>
class AqDev {
 public:
  AqDev() = default;
  AqDev(const AqDev &) = delete;
  AqDev &operator=(const AqDev &) = delete;
  AqDev(AqDev &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  AqDev &operator=(AqDev &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; bytes_ = o.bytes_;
      o.p_ = nullptr; o.bytes_ = 0;
    }
    return *this;
  }
  ~AqDev() { reset(); }

  int alloc(size_t count) {
    reset();
    AQ_HIP(hipMalloc((void **)&p_, count * sizeof(T)));
    bytes_ = (int64_t)(count * sizeof(T));
    aq_live_device_bytes += bytes_;
    return AQ_OK;
  }
  int alloc_zeroed(size_t count) {
    AQ_TRY(alloc(count));
    AQ_HIP(hipMemset(p_, 0, count * sizeof(T)));
    return AQ_OK;
  }
  T *get() const { return p_; }
  T *release() {
    T *r = p_;
    aq_live_device_bytes -= bytes_;
    p_ = nullptr; bytes_ = 0;
    return r;
  }
  void reset() {
    if (p_) hipFree(release());
  }

 private:
  T *p_ = nullptr;
  int64_t bytes_ = 0;
};

// --------------------------------------------- functions shared by the units ----
// IEEE double -> key whose unsigned order is the order of the values (negative: all bits flipped; otherwise: sign bit set):
// the radix select of aq_summary.hip and the column sort of aq_ytrans_kernels.h
__host__ __device__ inline uint64_t aq_key_of_bits(uint64_t b) { return (b >> 63) ? ~b : (b | 0x8000000000000000ull); }

struct aq_vb;

// aq_ops.hip
int aq_probe_dmode(int *dmode);   // accumulator layout of v_mfma_f64_16x16x4 on the current device (probed once per process)
int aq_need_acc_layout(const char *who);   // ... and the error of entry `who` unless it is row = (lane >> 4) + 4 reg

// aq_vb_sweep.hip
int aq_check_chain_error(aq_vb *s);   // a bounded wait inside a sweep kernel expired: the handle has failed
void aq_resolve_events(aq_vb *s);     // folds the finished sweeps' event pairs into core_ms_acc / core_launches
bool aq_all_equal_1(double c);        // isTRUE(all.equal(c, 1)), R/update_vb.R:219

// aq_vb_query.hip (aq_layout_kernels.h)
// (rows x q) column-major src -> trait-tiled dst [ntile][rows_pad][16], zero padded; nan_to_zero: NaN -> 0.  Asynchronous.
int aq_tile_from_colmajor(const double *src, double *dst, int rows, int q, int rows_pad, int ntile, int nan_to_zero);
// trait-tiled src (times mul, if given) of handle s -> a fresh (rows x q) column-major buffer in *out.  Asynchronous.
int aq_colmajor_copy(const aq_vb *s, const double *src, const double *mul, int rows, int rows_pad, AqDev<double> *out);

// aq_postproc.hip (hipCUB sort / scan)
struct aq_shard_sorted;
int aq_bfdr_device(const double *d_ppi, double *d_fdr, int64_t len);
int aq_row_count_device(const double *d_m, int64_t *d_rs, int p, int q, double thres, int lt);
int aq_shard_sort(const double *d_ppi, int64_t len, aq_shard_sorted **out);
int aq_shard_query(const aq_shard_sorted *s, double c, double out[5]);
int aq_shard_rows(const aq_shard_sorted *s, int64_t upto, int64_t t0, int64_t take, int p, int64_t *rs_host);
void aq_shard_free(aq_shard_sorted *s);
int aq_shard_pairs(const aq_shard_sorted *sh, int64_t upto, int64_t t0, int64_t take, const double *gam_tile, const double *mu_tile,
                   int p, int q, int p_pad, int32_t *snp, int32_t *trait, double *ppi, double *beta);
int aq_pairs_device(const double *d_cm, const double *src_ppi, const double *src_mul, int p, int q, int p_pad, int tiled, double thres,
                    int fdr_adjust, int64_t cap, int32_t *snp, int32_t *trait, double *ppi, double *beta, double *fdr,
                    int64_t *n_pairs);

// aq_summary.hip (radix select and moments of the p x q values)
int aq_moments_device(const aq_pair_src &src, size_t n_el, aq_moments *out);
int aq_rsel_hist_device(const aq_pair_src &src, size_t n_el, int n_prefix, const uint64_t *prefix, int shift, int64_t *hist);
int aq_order_stats_device(const aq_pair_src &src, size_t n_el, int n_ranks, const int64_t *ranks, double *out, aq_moments *mom,
                          const char *who);
