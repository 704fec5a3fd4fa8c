// Certified dual lower bound from trace bounds: the per-block norm kernels and the trace-bound detection.  lower_bound.h has the
// contracts; DESIGN.md, "Certified lower bound", the mathematics.
//
// lb_block_norms_kernel reads M and P once (16 B per slot) and writes [||M_k||^2, ||P_k||^2] per block.  The owner of a range of slots
// is a GROUP of W lanes with a fixed element-to-lane map: where M and P share their 16-byte phase, lane 0 takes a misaligned first
// slot, lane j the pairs j, j + W, ... (one 16-byte load per vector) and lane 0 an odd last slot; else lane j takes slots j, j + W, ...
//   small regime  W = 16 (one DPP row; four blocks per wavefront) for blocks of up to kLbRowMax slots, W = 64 up to kLbChunk:
//                 the group owns the whole block; wavefronts stride over the task list, so the grid does not enter the sums
//   large regime  a block beyond kLbChunk slots is cut into chunks of kLbChunk, W = 256: one workgroup per chunk writes a partial,
//                 and lb_large_final_kernel adds a block's chunks in index order (one wavefront per block)
// Sums inside a group go through the DPP butterfly of wave_sum (wave_reduce.h), the waves of a workgroup are added in order.  No atomics:
// the results are bit-identical from run to run.
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

// partial sums of lane j of a group of W lanes over slots [0, len) of m and p
__device__ __forceinline__ void range_acc(const double* __restrict__ m, const double* __restrict__ p, long long len, int j, int W, int vec,
                                          double& sm, double& sp) {
  if (vec) {
    const long long head = (((reinterpret_cast<uintptr_t>(m) >> 3) & 1) && len > 0) ? 1 : 0;
    const long long np = (len - head) >> 1;
    const double2* m2 = reinterpret_cast<const double2*>(m + head);
    const double2* p2 = reinterpret_cast<const double2*>(p + head);
    for (long long q = j; q < np; q += W) {
      const double2 a = m2[q], b = p2[q];
      sm += a.x * a.x; sm += a.y * a.y;
      sp += b.x * b.x; sp += b.y * b.y;
    }
    if (j == 0) {
      if (head) { sm += m[0] * m[0]; sp += p[0] * p[0]; }
      const long long tail = head + 2 * np;
      if (tail < len) { sm += m[tail] * m[tail]; sp += p[tail] * p[tail]; }
    }
  } else {
    for (long long i = j; i < len; i += W) { sm += m[i] * m[i]; sp += p[i] * p[i]; }
  }
}

__global__ __launch_bounds__(kLbThreads) void lb_block_norms_kernel(LbNormArgs a, int nwg_small, int vec) {
  __shared__ double lds[4];
  if ((int)blockIdx.x < nwg_small) {
    // ---- small regime: a row of 16 lanes or the wavefront owns whole blocks
    const int lane = threadIdx.x & 63, row = lane >> 4;
    const int nw = nwg_small * (kLbThreads / 64);
    for (int t = (int)blockIdx.x * (kLbThreads / 64) + (threadIdx.x >> 6); t < a.nwave; t += nw) {      // wave-uniform
      const int4 task = reinterpret_cast<const int4*>(a.wave)[t];
      const bool wide = task.y == -2;
      const int k = wide ? task.x : (row == 0 ? task.x : row == 1 ? task.y : row == 2 ? task.z : task.w);
      const int W = wide ? 64 : 16, j = wide ? lane : (lane & 15);
      double sm = 0, sp = 0;
      if (k >= 0) {
        const long long off = a.off[k];
        range_acc(a.M + off, a.P + off, a.len[k], j, W, vec, sm, sp);
      }
      sm = row_sum(sm); sp = row_sum(sp);                   // every lane of the wavefront is here
      if (wide) { sm = rows_to_wave(sm); sp = rows_to_wave(sp); }
      if (j == 0 && k >= 0) { a.pairs[2 * (size_t)k] = sm; a.pairs[2 * (size_t)k + 1] = sp; }
    }
    return;
  }
  // ---- large regime: this workgroup reduces one chunk of a block
  const int c = (int)blockIdx.x - nwg_small;
  const int k = a.chunk[2 * (size_t)c];
  const long long first = (long long)a.chunk[2 * (size_t)c + 1] * kLbChunk;
  const long long off = a.off[k] + first, rest = a.len[k] - first, len = rest < kLbChunk ? rest : kLbChunk;
  double sm = 0, sp = 0;
  range_acc(a.M + off, a.P + off, len, threadIdx.x, kLbThreads, vec, sm, sp);
  sm = block_sum(sm, lds);
  sp = block_sum(sp, lds);
  if (threadIdx.x == 0) { a.cpart[2 * (size_t)c] = sm; a.cpart[2 * (size_t)c + 1] = sp; }
}

// second stage of the large regime: one wavefront per chunked block adds its chunks, lane l the chunks l, l + 64, ...
__global__ __launch_bounds__(64) void lb_large_final_kernel(const int* large, const double* cpart, double* pairs) {
  const int k = large[3 * (size_t)blockIdx.x], first = large[3 * (size_t)blockIdx.x + 1], cnt = large[3 * (size_t)blockIdx.x + 2];
  double sm = 0, sp = 0;
  for (int c = threadIdx.x; c < cnt; c += 64) { sm += cpart[2 * (size_t)(first + c)]; sp += cpart[2 * (size_t)(first + c) + 1]; }
  sm = wave_sum(sm); sp = wave_sum(sp);
  if (threadIdx.x == 0) { pairs[2 * (size_t)k] = sm; pairs[2 * (size_t)k + 1] = sp; }
}

constexpr long long kDotStride = (long long)kLbDotSlots * kLbThreads;
__global__ __launch_bounds__(kLbThreads) void lb_dot_kernel(long long n, const double* __restrict__ x, const double* __restrict__ y, double* partials) {
  __shared__ double lds[4];
  double s = 0;
  for (long long i = (long long)blockIdx.x * kLbThreads + threadIdx.x; i < n; i += kDotStride) s += x[i] * y[i];
  s = block_sum(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(kLbThreads) void lb_combine_kernel(int nblk, const double* __restrict__ pairs, const double* __restrict__ R,
                                                                const long long* __restrict__ len, const int* __restrict__ blk,
                                                                const double* dot_partials, double* out4) {
  __shared__ double lds[4];
  __shared__ double best_v[kLbThreads];
  __shared__ int best_k[kLbThreads];
  double s = 0, bv = -1.0;
  int bk = -1;
  for (int k = threadIdx.x; k < nblk; k += kLbThreads) {
    double nu = sqrt(pairs[2 * (size_t)k + 1]);
    if (blk[k] >= 0) nu += kLbProjErr * sqrt((double)len[k]) * sqrt(pairs[2 * (size_t)k]);
    const double term = R[k] * nu;
    s += term;
    if (term > bv) { bv = term; bk = k; }        // the first of equal terms
  }
  s = block_sum(s, lds);
  const double d = block_sum(dot_partials && threadIdx.x < kLbDotSlots ? dot_partials[threadIdx.x] : 0.0, lds);
  best_v[threadIdx.x] = bv; best_k[threadIdx.x] = bk;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < kLbThreads; ++t)
      if (best_k[t] >= 0 && (best_v[t] > bv || (best_v[t] == bv && best_k[t] < bk))) { bv = best_v[t]; bk = best_k[t]; }
    out4[0] = s; out4[1] = (double)bk; out4[2] = bk >= 0 ? bv : 0.0; out4[3] = d;
  }
}

bool same_phase(const void* a, const void* b) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return (x & 7) == 0 && (y & 7) == 0 && (x & 15) == (y & 15);
}

}  // namespace

int lb_build_tasks(int nblk, const long long* len, LbTasks* out) {
  if (nblk < 0 || (nblk > 0 && !len) || !out) { set_error("lb_build_tasks: invalid argument"); return CUADMM_ERR_INVALID; }
  out->wave.clear(); out->chunk.clear(); out->large.clear();
  int fill = 4;                       // rows used in the open 16-lane task
  size_t open = 0;
  for (int k = 0; k < nblk; ++k) {
    if (len[k] < 0) { set_error("lb_build_tasks: block %d has a negative length", k); return CUADMM_ERR_INVALID; }
    if (len[k] == 0) continue;
    if (len[k] <= kLbRowMax) {
      if (fill == 4) { open = out->wave.size(); out->wave.insert(out->wave.end(), 4, -1); fill = 0; }
      out->wave[open + fill++] = k;
    } else if (len[k] <= kLbChunk) {
      const int t[4] = {k, -2, -2, -2};
      out->wave.insert(out->wave.end(), t, t + 4);
    } else {
      const long long nc = (len[k] + kLbChunk - 1) / kLbChunk;
      if (nc > (1LL << 30) || (long long)out->nchunk() + nc > (1LL << 30)) { set_error("lb_build_tasks: too many chunks"); return CUADMM_ERR_INVALID; }
      const int t[3] = {k, out->nchunk(), (int)nc};
      out->large.insert(out->large.end(), t, t + 3);
      for (int c = 0; c < (int)nc; ++c) { out->chunk.push_back(k); out->chunk.push_back(c); }
    }
  }
  return CUADMM_OK;
}

int launch_lb_block_norms(const LbNormArgs& a, hipStream_t st) {
  if (!a.M || !a.P || !a.pairs || a.nwave < 0 || a.nchunk < 0 || a.nlarge < 0 || (a.nwave > 0 && !a.wave) ||
      (a.nchunk > 0 && (!a.chunk || !a.large || !a.cpart || a.nlarge < 1)) || ((a.nwave > 0 || a.nchunk > 0) && (!a.off || !a.len))) {
    set_error("lb_block_norms: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  if (a.nwave == 0 && a.nchunk == 0) return CUADMM_OK;
  const int per = kLbThreads / 64;
  const int nwg_small = std::min((a.nwave + per - 1) / per, kLbSmallGrid);
  hipLaunchKernelGGL(lb_block_norms_kernel, dim3((unsigned)(nwg_small + a.nchunk)), dim3(kLbThreads), 0, st, a, nwg_small, same_phase(a.M, a.P) ? 1 : 0);
  if (a.nlarge > 0) hipLaunchKernelGGL(lb_large_final_kernel, dim3((unsigned)a.nlarge), dim3(64), 0, st, a.large, a.cpart, a.pairs);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_lb_dot(long long n, const double* a, const double* b, double* partials, hipStream_t st) {
  if (n < 0 || (n > 0 && (!a || !b)) || !partials) { set_error("lb_dot: invalid argument"); return CUADMM_ERR_INVALID; }
  hipLaunchKernelGGL(lb_dot_kernel, dim3(kLbDotSlots), dim3(kLbThreads), 0, st, n, a, b, partials);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_lb_combine(int nblk, const double* pairs, const double* R, const long long* len, const int* blk, const double* dot_partials,
                      double* out4, hipStream_t st) {
  if (nblk < 0 || (nblk > 0 && (!pairs || !R || !len || !blk)) || !out4) { set_error("lb_combine: invalid argument"); return CUADMM_ERR_INVALID; }
  hipLaunchKernelGGL(lb_combine_kernel, dim3(1), dim3(kLbThreads), 0, st, nblk, pairs, R, len, blk, dot_partials, out4);
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
