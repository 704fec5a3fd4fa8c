// KKT and DIMACS report of any point (cuadmm_evaluate): the per-block statistics kernel and the reductions behind it.  evaluate.h has
// the contracts; DESIGN.md, "Evaluation of a point", the definitions.
//
// ev_block_stats_kernel reads X, S, PX, PS and Rd1 once (40 B per slot) and writes six sums per block.  Ownership, element-to-lane map
// and task lists are those of lb_block_norms_kernel (lower_bound.hip): a row of 16 lanes owns a block of up to kLbRowMax slots, the
// wavefront one of up to kLbChunk, a workgroup a chunk of a longer one, whose chunks ev_large_final_kernel adds in index order.  Where
// the five vectors share their 16-byte phase, lane 0 takes a misaligned first slot, lane j the pairs j, j + W, ... (one 16-byte load
// per vector) and lane 0 an odd last slot; else lane j takes slots j, j + W, ...  An svec block of n (n + 1) / 2 slots starts at an
// odd slot as often as not, so the head is the common case.  No atomics, nothing written but the sums (and the chunk partials).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "evaluate.h"
#include "device_util.h"
#include "wave_reduce.h"

namespace cuadmm {
namespace {

struct Acc6 {
  double v[kEvSums] = {0, 0, 0, 0, 0, 0};
};

// one slot: x, s, their projections and Rd1; free_blk: an unconstrained block (no cone violation of x, all of s is one)
__device__ __forceinline__ void slot_acc(Acc6& a, double x, double s, double px, double ps, double r1, bool free_blk) {
  const double dx = free_blk ? 0.0 : px - x;
  const double ds = free_blk ? s : ps - s;
  const double rd = r1 + s;
  a.v[0] += x * x;
  a.v[1] += dx * dx;
  a.v[2] += s * s;
  a.v[3] += ds * ds;
  a.v[4] += x * s;
  a.v[5] += rd * rd;
}

// partial sums of lane j of a group of W lanes over slots [first, first + len) of the five vectors
__device__ __forceinline__ void range_acc(const EvStatArgs& g, long long first, long long len, int j, int W, int vec, bool free_blk, Acc6& a) {
  const double *x = g.X + first, *s = g.S + first, *px = g.PX + first, *ps = g.PS + first, *r1 = g.Rd1 + first;
  if (vec) {
    const long long head = (((reinterpret_cast<uintptr_t>(x) >> 3) & 1) && len > 0) ? 1 : 0;
    const long long np = (len - head) >> 1;
    const double2 *x2 = reinterpret_cast<const double2*>(x + head), *s2 = reinterpret_cast<const double2*>(s + head);
    const double2 *px2 = reinterpret_cast<const double2*>(px + head), *ps2 = reinterpret_cast<const double2*>(ps + head);
    const double2* r2 = reinterpret_cast<const double2*>(r1 + head);
    for (long long q = j; q < np; q += W) {
      const double2 vx = x2[q], vs = s2[q], vpx = px2[q], vps = ps2[q], vr = r2[q];
      slot_acc(a, vx.x, vs.x, vpx.x, vps.x, vr.x, free_blk);
      slot_acc(a, vx.y, vs.y, vpx.y, vps.y, vr.y, free_blk);
    }
    if (j == 0) {
      if (head) slot_acc(a, x[0], s[0], px[0], ps[0], r1[0], free_blk);
      const long long tail = head + 2 * np;
      if (tail < len) slot_acc(a, x[tail], s[tail], px[tail], ps[tail], r1[tail], free_blk);
    }
  } else {
    for (long long i = j; i < len; i += W) slot_acc(a, x[i], s[i], px[i], ps[i], r1[i], free_blk);
  }
}

__global__ __launch_bounds__(kLbThreads) void ev_block_stats_kernel(EvStatArgs a, int nwg_small, int vec) {
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
      Acc6 acc;
      if (k >= 0) range_acc(a, a.off[k], a.len[k], j, W, vec, a.blk[k] < 0, acc);
#pragma unroll
      for (int q = 0; q < kEvSums; ++q) {                   // every lane of the wavefront is here
        double v = row_sum(acc.v[q]);
        if (wide) v = rows_to_wave(v);
        if (j == 0 && k >= 0) a.sums[kEvSums * (size_t)k + q] = v;
      }
    }
    return;
  }
  // ---- large regime: this workgroup reduces one chunk of a block
  const int c = (int)blockIdx.x - nwg_small;
  const int k = a.chunk[2 * (size_t)c];
  const long long first = (long long)a.chunk[2 * (size_t)c + 1] * kLbChunk;
  const long long rest = a.len[k] - first, len = rest < kLbChunk ? rest : kLbChunk;
  Acc6 acc;
  range_acc(a, a.off[k] + first, len, threadIdx.x, kLbThreads, vec, a.blk[k] < 0, acc);
#pragma unroll
  for (int q = 0; q < kEvSums; ++q) {
    const double v = block_sum(acc.v[q], lds);
    if (threadIdx.x == 0) a.cpart[kEvSums * (size_t)c + q] = v;
  }
}

// second stage of the large regime: one wavefront per chunked block adds its chunks, lane l the chunks l, l + 64, ...
__global__ __launch_bounds__(64) void ev_large_final_kernel(const int* large, const double* cpart, double* sums) {
  const int k = large[3 * (size_t)blockIdx.x], first = large[3 * (size_t)blockIdx.x + 1], cnt = large[3 * (size_t)blockIdx.x + 2];
  double s[kEvSums] = {0, 0, 0, 0, 0, 0};
  for (int c = threadIdx.x; c < cnt; c += 64)
#pragma unroll
    for (int q = 0; q < kEvSums; ++q) s[q] += cpart[kEvSums * (size_t)(first + c) + q];
#pragma unroll
  for (int q = 0; q < kEvSums; ++q) {
    const double v = wave_sum(s[q]);
    if (threadIdx.x == 0) sums[kEvSums * (size_t)k + q] = v;
  }
}

constexpr long long kRpStride = (long long)kLbDotSlots * kLbThreads;
__global__ __launch_bounds__(kLbThreads) void ev_rp_kernel(int m, const double* __restrict__ ax, const double* __restrict__ b, const double* __restrict__ normA,
                                                           double bscale, double* partials) {
  __shared__ double lds[4];
  double s = 0;
  for (long long i = (long long)blockIdx.x * kLbThreads + threadIdx.x; i < m; i += kRpStride) {
    const double ro = normA[i] * (b[i] - ax[i]) * bscale;      // the stopping test's ||Rp|| in the caller's units (engine.hip, Step 5)
    s += ro * ro;
  }
  s = block_sum(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(kLbThreads) void ev_combine_kernel(int nblk, const double* __restrict__ sums, const double* cx_part, const double* by_part,
                                                                const double* rp_part, double* out8) {
  __shared__ double lds[4];
  static_assert(kLbDotSlots == kLbThreads, "one partial per thread");
  double vx = 0, vs = 0, xs = 0, rd = 0;
  for (int k = threadIdx.x; k < nblk; k += kLbThreads) {
    const double* q = sums + kEvSums * (size_t)k;
    vx += q[1]; vs += q[3]; xs += q[4]; rd += q[5];
  }
  vx = block_sum(vx, lds); vs = block_sum(vs, lds); xs = block_sum(xs, lds); rd = block_sum(rd, lds);
  const double cx = block_sum(cx_part[threadIdx.x], lds), by = block_sum(by_part[threadIdx.x], lds), rp = block_sum(rp_part[threadIdx.x], lds);
  if (threadIdx.x == 0) {
    out8[0] = vx; out8[1] = vs; out8[2] = xs; out8[3] = rd; out8[4] = cx; out8[5] = by; out8[6] = rp; out8[7] = 0.0;
  }
}

bool same_phase5(const EvStatArgs& a) {
  const uintptr_t p[5] = {reinterpret_cast<uintptr_t>(a.X), reinterpret_cast<uintptr_t>(a.S), reinterpret_cast<uintptr_t>(a.PX),
                          reinterpret_cast<uintptr_t>(a.PS), reinterpret_cast<uintptr_t>(a.Rd1)};
  for (uintptr_t v : p)
    if ((v & 7) != 0 || (v & 15) != (p[0] & 15)) return false;
  return true;
}

}  // namespace

int launch_ev_block_stats(const EvStatArgs& a, hipStream_t st) {
  if (!a.X || !a.S || !a.PX || !a.PS || !a.Rd1 || !a.sums || a.nwave < 0 || a.nchunk < 0 || a.nlarge < 0 || (a.nwave > 0 && !a.wave) ||
      (a.nchunk > 0 && (!a.chunk || !a.large || !a.cpart || a.nlarge < 1)) || ((a.nwave > 0 || a.nchunk > 0) && (!a.off || !a.len || !a.blk))) {
    set_error("ev_block_stats: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  if (a.nwave == 0 && a.nchunk == 0) return CUADMM_OK;
  const int per = kLbThreads / 64;
  const int nwg_small = std::min((a.nwave + per - 1) / per, kLbSmallGrid);
  hipLaunchKernelGGL(ev_block_stats_kernel, dim3((unsigned)(nwg_small + a.nchunk)), dim3(kLbThreads), 0, st, a, nwg_small, same_phase5(a) ? 1 : 0);
  if (a.nlarge > 0) hipLaunchKernelGGL(ev_large_final_kernel, dim3((unsigned)a.nlarge), dim3(64), 0, st, a.large, a.cpart, a.sums);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_ev_rp(int m, const double* ax, const double* b, const double* normA, double bscale, double* partials, hipStream_t st) {
  if (m < 0 || (m > 0 && (!ax || !b || !normA)) || !partials) { set_error("ev_rp: invalid argument"); return CUADMM_ERR_INVALID; }
  hipLaunchKernelGGL(ev_rp_kernel, dim3(kLbDotSlots), dim3(kLbThreads), 0, st, m, ax, b, normA, bscale, partials);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_ev_combine(int nblk, const double* sums, const double* cx_part, const double* by_part, const double* rp_part, double* out8, hipStream_t st) {
  if (nblk < 0 || (nblk > 0 && !sums) || !cx_part || !by_part || !rp_part || !out8) { set_error("ev_combine: invalid argument"); return CUADMM_ERR_INVALID; }
  hipLaunchKernelGGL(ev_combine_kernel, dim3(1), dim3(kLbThreads), 0, st, nblk, sums, cx_part, by_part, rp_part, out8);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

}  // namespace cuadmm
