// The factor layout every low-rank call speaks (cuadmm_lowrank's L_out, the L of cuadmm_set_lowrank, V and W of cuadmm_block_multiply, L and
// G of cuadmm_lowrank_grad, L and D of cuadmm_lowrank_line) and the one check of a caller's factor buffers.  DESIGN.md, "The factor layout".
// Host only, no HIP include: plain g++ compiles it.
//
// For a cap rmax, PSD block k of size n_k holds factor_cols(n_k, rmax) = min(n_k, rmax) columns of n_k doubles each, column by column, and
// starts at the prefix sum of those products over the PSD blocks before it; unconstrained blocks (negative size) occupy nothing.  A
// caller's ranks[k] <= factor_cols says how many of the columns are read; the others may hold anything, NaN included.
#pragma once
#include <cmath>
#include <vector>

#include "common.h"

namespace cuadmm {

constexpr int kFactorMaxBlock = 8192;     // = kMaxBlockSize (device_util.h; report_plans.h asserts it)

inline int factor_cols(int n, int rmax) { return n < rmax ? n : rmax; }

// loff (nblk + 1 entries): first double of block k's factor; loff[nblk] is the buffer's length.  who: the caller's name in the messages.
inline int factor_offsets(const char* who, int nblk, const int* blk, int rmax, std::vector<long long>* loff) {
  if (nblk < 0 || (nblk > 0 && !blk) || rmax < 1 || rmax > kFactorMaxBlock || !loff) { set_error("%s: invalid argument", who); return CUADMM_ERR_INVALID; }
  loff->assign((size_t)nblk + 1, 0);
  for (int k = 0; k < nblk; ++k) {
    const int n = blk[k];
    if (n == 0 || n > kFactorMaxBlock) { set_error("%s: block %d has size %d", who, k, n); return CUADMM_ERR_INVALID; }
    (*loff)[k + 1] = (*loff)[k] + (n > 0 ? (long long)n * factor_cols(n, rmax) : 0);
  }
  return CUADMM_OK;
}

// A caller's factors before anything is staged, block by block in this order: 0 <= ranks[k] <= factor_cols, a buffer that is null while a
// rank is positive, an entry of a read column that is not finite (columns >= ranks[k] are not looked at; neither is the rank of an
// unconstrained block).  One buffer (name1 = null) or two of one layout: then a null or an entry is reported with its buffer's name, the
// first buffer's first.  *blocks, *rank_sum (may be null): the PSD blocks and the sum of their ranks.
inline int check_factors(const char* who, int nblk, const int* blk, const int* ranks, int rmax, const char* name0, const double* buf0, const char* name1,
                         const double* buf1, double* blocks, double* rank_sum) {
  std::vector<long long> loff;
  int rc = factor_offsets(who, nblk, blk, rmax, &loff);
  if (rc) return rc;
  if (!ranks) { set_error("%s: ranks is null", who); return CUADMM_ERR_INVALID; }
  double nb = 0, rs = 0;
  for (int k = 0; k < nblk; ++k) {
    const int n = blk[k];
    if (n <= 0) continue;
    const int rc_k = factor_cols(n, rmax), r = ranks[k];
    const long long at = loff[k];
    if (r < 0 || r > rc_k) { set_error("%s: block %d of size %d has rank %d, allowed are 0 to %d", who, k, n, r, rc_k); return CUADMM_ERR_INVALID; }
    if (r > 0 && (!buf0 || (name1 && !buf1))) { set_error("%s: %s is null and block %d has rank %d", who, buf0 ? name1 : name0, k, r); return CUADMM_ERR_INVALID; }
    for (long long e = at, end = at + (long long)n * r; e < end; ++e) {
      const bool bad0 = !std::isfinite(buf0[e]);
      if (!bad0 && !(name1 && !std::isfinite(buf1[e]))) continue;
      if (name1) set_error("%s: block %d, row %lld of column %lld of %s is not finite", who, k, (e - at) % n, (e - at) / n, bad0 ? name0 : name1);
      else set_error("%s: block %d, row %lld of column %lld is not finite", who, k, (e - at) % n, (e - at) / n);
      return CUADMM_ERR_INVALID;
    }
    nb += 1;
    rs += r;
  }
  if (blocks) *blocks = nb;
  if (rank_sum) *rank_sum = rs;
  return CUADMM_OK;
}

}  // namespace cuadmm
