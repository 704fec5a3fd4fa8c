// Certified dual lower bound from trace bounds: the per-block norms, the combine kernel and the trace-bound detection.  lower_bound.h has
// the contracts; DESIGN.md, "Certified lower bound", the mathematics.
//
// The per-block norms are block_reduce.h's skeleton with two vectors and two sums: M and P are read once (16 B per slot) and
// [||M_k||^2, ||P_k||^2] written per block; b'y is its slot-partial kernel over x[i] y[i].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "lower_bound.h"
#include "device_util.h"
#include "wave_reduce.h"

namespace cuadmm {
namespace {

struct LbBlockNorms {
  static constexpr int V = 2, N = 2;
  static constexpr bool kFlag = false;
  static constexpr const char* kName = "lb_block_norms";
  const double* p[V];      // M, P
  __device__ __forceinline__ void add(double (&s)[N], const double (&v)[V], bool) const {
    s[0] += v[0] * v[0];
    s[1] += v[1] * v[1];
  }
};

struct DotTerm {
  const double *x, *y;
  __device__ __forceinline__ void add(double& s, long long i) const { s += x[i] * y[i]; }
};

__global__ __launch_bounds__(kBrThreads) void lb_combine_kernel(int nblk, const double* __restrict__ pairs, const double* __restrict__ R,
                                                                const long long* __restrict__ len, const int* __restrict__ blk,
                                                                const double* dot_partials, double* out4) {
  __shared__ double lds[4];
  __shared__ double best_v[kBrThreads];
  __shared__ int best_k[kBrThreads];
  double s = 0, bv = -1.0;
  int bk = -1;
  for (int k = threadIdx.x; k < nblk; k += kBrThreads) {
    double nu = sqrt(pairs[2 * (size_t)k + 1]);
    if (blk[k] >= 0) nu += kLbProjErr * sqrt((double)len[k]) * sqrt(pairs[2 * (size_t)k]);
    const double term = R[k] * nu;
    s += term;
    if (term > bv) { bv = term; bk = k; }        // the first of equal terms
  }
  s = block_sum(s, lds);
  const double d = block_sum(dot_partials && threadIdx.x < kBrSlots ? dot_partials[threadIdx.x] : 0.0, lds);
  best_v[threadIdx.x] = bv; best_k[threadIdx.x] = bk;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < kBrThreads; ++t)
      if (best_k[t] >= 0 && (best_v[t] > bv || (best_v[t] == bv && best_k[t] < bk))) { bv = best_v[t]; bk = best_k[t]; }
    out4[0] = s; out4[1] = (double)bk; out4[2] = bk >= 0 ? bv : 0.0; out4[3] = d;
  }
}

}  // namespace

int launch_lb_block_norms(const double* M, const double* P, const BlockTasksView& t, double* cpart, double* pairs, hipStream_t st) {
  return launch_block_reduce(LbBlockNorms{{M, P}}, t, cpart, pairs, st);
}

int launch_lb_dot(long long n, const double* a, const double* b, double* partials, hipStream_t st) {
  if (n < 0 || (n > 0 && (!a || !b)) || !partials) { set_error("lb_dot: invalid argument"); return CUADMM_ERR_INVALID; }
  return launch_slot_partials(n, DotTerm{a, b}, partials, st);
}

int launch_lb_combine(int nblk, const double* pairs, const double* R, const long long* len, const int* blk, const double* dot_partials,
                      double* out4, hipStream_t st) {
  if (nblk < 0 || (nblk > 0 && (!pairs || !R || !len || !blk)) || !out4) { set_error("lb_combine: invalid argument"); return CUADMM_ERR_INVALID; }
  hipLaunchKernelGGL(lb_combine_kernel, dim3(1), dim3(kBrThreads), 0, st, nblk, pairs, R, len, blk, dot_partials, out4);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

// Rule 1: a constraint whose entries are exactly the n diagonal slots of ONE PSD block, all with the same value c, fixes
// tr X_k = b_j / c.  Rule 2: constraints with a single entry, on a diagonal slot, fix that diagonal entry; a block with every
// diagonal entry fixed has the sum as its trace.  The smaller of the two; a negative value anywhere in a rule: that rule finds nothing.
int lb_trace_bounds_detect(int vec_len, int con_num, const int* At_cp, const int* At_ri, const double* At_vx, const int* b_idx,
                           const double* b_val, int b_nnz, const int* blk, int mat_num, double* R_out) {
  if (vec_len < 0 || con_num < 0 || mat_num < 0 || b_nnz < 0 || !At_cp || (mat_num > 0 && (!blk || !R_out)) || (b_nnz > 0 && (!b_idx || !b_val)) ||
      (At_cp[con_num] > 0 && (!At_ri || !At_vx))) {
    set_error("trace_bounds_detect: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  std::vector<long long> off((size_t)mat_num + 1, 0);
  for (int k = 0; k < mat_num; ++k) off[(size_t)k + 1] = off[k] + blk_svec_len(blk[k]);
  if (off[mat_num] != vec_len) { set_error("trace_bounds_detect: the blocks cover %lld slots, vec_len is %d", off[mat_num], vec_len); return CUADMM_ERR_INVALID; }
  std::vector<double> b((size_t)con_num, 0.0);
  for (int q = 0; q < b_nnz; ++q) {
    if (b_idx[q] < 0 || b_idx[q] >= con_num) { set_error("trace_bounds_detect: b index %d outside [0, %d)", b_idx[q], con_num); return CUADMM_ERR_INVALID; }
    b[b_idx[q]] = b_val[q];
  }
  // slot -> (block, row if the slot is a diagonal one, else -1)
  auto locate = [&](long long slot, int* k_out, int* diag_out) {
    const int k = (int)(std::upper_bound(off.begin(), off.end(), slot) - off.begin()) - 1;
    *k_out = k;
    *diag_out = -1;
    if (blk[k] < 0) return;
    const long long t = slot - off[k];
    long long i = (long long)((std::sqrt(8.0 * (double)t + 1.0) - 1.0) / 2.0);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    if (t == i * (i + 1) / 2 + i) *diag_out = (int)i;
  };
  const double none = -1.0;
  std::vector<double> r1((size_t)mat_num, none);
  std::vector<std::vector<double>> fixed((size_t)mat_num);     // rule 2: the fixed diagonal entries (NaN: not fixed)
  const double nan = std::nan("");
  for (int j = 0; j < con_num; ++j) {
    const int p0 = At_cp[j], p1 = At_cp[j + 1];
    if (p1 <= p0) continue;
    for (int p = p0; p < p1; ++p)
      if (At_ri[p] < 0 || At_ri[p] >= vec_len) { set_error("trace_bounds_detect: row index %d outside [0, %d)", At_ri[p], vec_len); return CUADMM_ERR_INVALID; }
    int k0, d0;
    locate(At_ri[p0], &k0, &d0);
    if (blk[k0] < 0 || d0 < 0 || At_vx[p0] == 0.0) continue;
    const int n = blk[k0];
    if (p1 - p0 == 1) {            // rule 2
      if (fixed[k0].empty()) fixed[k0].assign((size_t)n, nan);
      fixed[k0][d0] = b[j] / At_vx[p0];
    }
    if (p1 - p0 == n) {            // rule 1 (n = 1: both rules see the row)
      std::vector<char> seen((size_t)n, 0);
      bool ok = true;
      for (int p = p0; p < p1 && ok; ++p) {
        int k, d;
        locate(At_ri[p], &k, &d);
        ok = k == k0 && d >= 0 && !seen[d] && At_vx[p] == At_vx[p0];
        if (ok) seen[d] = 1;
      }
      const double tr = b[j] / At_vx[p0];
      if (ok && tr >= 0 && std::isfinite(tr) && (r1[k0] < 0 || tr < r1[k0])) r1[k0] = tr;
    }
  }
  for (int k = 0; k < mat_num; ++k) {
    double r = blk[k] < 0 ? none : r1[k];
    if (blk[k] > 0 && !fixed[k].empty()) {
      long double sum = 0;
      bool ok = true;
      for (double v : fixed[k]) { ok = ok && v >= 0 && std::isfinite(v); sum += v; }      // (NaN >= 0 is false: an entry not fixed)
      if (ok && (r < 0 || (double)sum < r)) r = (double)sum;
    }
    R_out[k] = r;
  }
  return CUADMM_OK;
}

}  // namespace cuadmm
