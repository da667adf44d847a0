// aq_pair_src.h -- where the p x q posterior values are read from, shared by aq_postproc.hip (table of associations) and
// aq_summary.hip (order statistics): the trait-tiled state of a handle [(tile p_pad + j) 16 + k % 16] or a plain array.
#ifndef AQ_PAIR_SRC_H_
#define AQ_PAIR_SRC_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

struct aq_pair_src {
  const double *ppi;   // tiled gam, or p x q column-major PPIs
  const double *mul;   // tiled mu_beta_vb (beta = ppi * mul), or p x q column-major beta (copied), or NULL
  int p, q, p_pad, tiled;
};
// storage element e -> column-major position j + p k; false for the padding rows / traits of a tiled array
__device__ inline bool aq_src_pos(const aq_pair_src &s, size_t e, uint64_t *pos) {
  if (!s.tiled) { *pos = e; return true; }
  const size_t row = e >> 4, tile = row / (size_t)s.p_pad, j = row - tile * (size_t)s.p_pad, kk = tile * 16 + (e & 15);
  if (j >= (size_t)s.p || kk >= (size_t)s.q) return false;
  *pos = j + (size_t)s.p * kk;
  return true;
}
// storage elements of the source: the tiles that hold a trait, padding included
static inline size_t aq_src_elements(const aq_pair_src &s, size_t len_plain) {
  return s.tiled ? (size_t)((s.q + 15) / 16) * (size_t)s.p_pad * 16 : len_plain;
}
#endif /* AQ_PAIR_SRC_H_ */
