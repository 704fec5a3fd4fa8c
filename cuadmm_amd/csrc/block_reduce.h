// Deterministic sums per block of an svec layout, over V vectors read once: the task lists, the kernel skeleton and its launcher,
// shared by the lower bound's block norms (lower_bound.hip) and the evaluation's block statistics (evaluate.hip); and the fixed-stride
// slot partials both use for their inner products.  An Op states what a slot contributes; everything else is here.
//
// The owner of a range of slots is a GROUP of W lanes with a fixed element-to-lane map: where the V vectors share their 16-byte phase,
// lane 0 takes a misaligned first slot, lane j the pairs j, j + W, ... (one 16-byte load per vector) and lane 0 an odd last slot; else
// lane j takes slots j, j + W, ...  An svec block of n (n + 1) / 2 slots starts at an odd slot as often as not: the head is the common case.
//   small regime  W = 16 (one DPP row; four blocks per wavefront) for blocks of up to kBrRowMax slots, W = 64 up to kBrChunk:
//                 the group owns the whole block; wavefronts stride over the task list, so the grid does not enter the sums
//   large regime  a block beyond kBrChunk slots is cut into chunks of kBrChunk, W = 256: one workgroup per chunk writes a partial,
//                 and block_reduce_final_kernel adds a block's chunks in index order (one wavefront per block)
// Sums inside a group go through the DPP butterfly of wave_sum (wave_reduce.h), the waves of a workgroup are added in order.  No atomics,
// nothing written but the sums and the chunk partials: the results are bit-identical from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "device_util.h"
#include "wave_reduce.h"

namespace cuadmm {

constexpr int kBrThreads = 256;
constexpr long long kBrRowMax = 128;     // a block of up to this many slots is owned by 16 lanes (one DPP row), four blocks per wavefront
constexpr long long kBrChunk = 8192;     // a block of up to this many slots is owned by one wavefront; a longer one is cut into chunks of
                                         // this length (even: a chunk starts in the 16-byte phase of its block), one workgroup each
constexpr int kBrSmallGrid = 2048;       // workgroups of the small regime at most (a wavefront strides over its tasks: whole blocks,
                                         // so the sums do not depend on the grid)
constexpr int kBrSlots = 256;            // workgroups = partial sums of a slot-partial kernel

// What the kernel walks, built on the host from the blocks' lengths.
struct BlockTasks {
  std::vector<int> wave;    // 4 per wavefront task: the blocks of its four 16-lane rows (-1: none), or {k, -2, -2, -2}: the wavefront owns block k
  std::vector<int> chunk;   // 2 per workgroup task: block, chunk index
  std::vector<int> large;   // 3 per chunked block: block, first workgroup task, chunks
  int nwave() const { return (int)(wave.size() / 4); }
  int nchunk() const { return (int)(chunk.size() / 2); }
  int nlarge() const { return (int)(large.size() / 3); }
};
inline int build_block_tasks(int nblk, const long long* len, BlockTasks* out) {
  if (nblk < 0 || (nblk > 0 && !len) || !out) { set_error("build_block_tasks: invalid argument"); return CUADMM_ERR_INVALID; }
  out->wave.clear(); out->chunk.clear(); out->large.clear();
  int fill = 4;                       // rows used in the open 16-lane task
  size_t open = 0;
  for (int k = 0; k < nblk; ++k) {
    if (len[k] < 0) { set_error("build_block_tasks: block %d has a negative length", k); return CUADMM_ERR_INVALID; }
    if (len[k] == 0) continue;
    if (len[k] <= kBrRowMax) {
      if (fill == 4) { open = out->wave.size(); out->wave.insert(out->wave.end(), 4, -1); fill = 0; }
      out->wave[open + fill++] = k;
    } else if (len[k] <= kBrChunk) {
      const int t[4] = {k, -2, -2, -2};
      out->wave.insert(out->wave.end(), t, t + 4);
    } else {
      const long long nc = (len[k] + kBrChunk - 1) / kBrChunk;
      if (nc > (1LL << 30) || (long long)out->nchunk() + nc > (1LL << 30)) { set_error("build_block_tasks: too many chunks"); return CUADMM_ERR_INVALID; }
      const int t[3] = {k, out->nchunk(), (int)nc};
      out->large.insert(out->large.end(), t, t + 3);
      for (int c = 0; c < (int)nc; ++c) { out->chunk.push_back(k); out->chunk.push_back(c); }
    }
  }
  return CUADMM_OK;
}

// The lists on the device, as the kernel takes them.
struct BlockTasksView {
  const long long *off, *len;       // per block: first slot and slots
  const int* blk;                   // per block: its size as in cuadmm_init; negative: unconstrained.  Read only for an Op with kFlag
  const int *wave, *chunk, *large;  // BlockTasks
  int nwave, nchunk, nlarge;
};

// An Op is passed to the kernel by value and states
//   V, N                 vectors read per slot, sums per block
//   kFlag                whether add() wants to know that the block is an unconstrained one (blk[k] < 0); else blk is never read
//   kName                for the launcher's error text
//   const double* p[V]   the vectors
//   add(s, v, flag)      __device__ __forceinline__: adds the terms of one slot, whose V values are v, to the N sums s
template <class Op>
__device__ __forceinline__ void br_add_slot(const Op& op, const double* const (&p)[Op::V], long long i, bool flag, double (&s)[Op::N]) {
  double v[Op::V];
#pragma unroll
  for (int q = 0; q < Op::V; ++q) v[q] = p[q][i];
  op.add(s, v, flag);
}

// partial sums of lane j of a group of W lanes over slots [first, first + len) of the V vectors
template <class Op>
__device__ __forceinline__ void br_range_acc(const Op& op, long long first, long long len, int j, int W, int vec, bool flag, double (&s)[Op::N]) {
  constexpr int V = Op::V;
  const double* p[V];
#pragma unroll
  for (int q = 0; q < V; ++q) p[q] = op.p[q] + first;
  if (vec) {
    const long long head = (((reinterpret_cast<uintptr_t>(p[0]) >> 3) & 1) && len > 0) ? 1 : 0;
    const long long np = (len - head) >> 1;
    for (long long i = j; i < np; i += W) {
      double2 d[V];
      double v[V];
#pragma unroll
      for (int q = 0; q < V; ++q) d[q] = reinterpret_cast<const double2*>(p[q] + head)[i];
#pragma unroll
      for (int q = 0; q < V; ++q) v[q] = d[q].x;
      op.add(s, v, flag);
#pragma unroll
      for (int q = 0; q < V; ++q) v[q] = d[q].y;
      op.add(s, v, flag);
    }
    if (j == 0) {
      if (head) br_add_slot(op, p, 0, flag, s);
      const long long tail = head + 2 * np;
      if (tail < len) br_add_slot(op, p, tail, flag, s);
    }
  } else {
    for (long long i = j; i < len; i += W) br_add_slot(op, p, i, flag, s);
  }
}

template <class Op>
__global__ __launch_bounds__(kBrThreads) void block_reduce_kernel(Op op, BlockTasksView t, double* cpart, double* out, int nwg_small, int vec) {
  constexpr int N = Op::N;
  __shared__ double lds[4];
  double s[N];
  if ((int)blockIdx.x < nwg_small) {
    // ---- small regime: a row of 16 lanes or the wavefront owns whole blocks
    const int lane = threadIdx.x & 63, row = lane >> 4;
    const int nw = nwg_small * (kBrThreads / 64);
    for (int u = (int)blockIdx.x * (kBrThreads / 64) + (threadIdx.x >> 6); u < t.nwave; u += nw) {      // wave-uniform
      const int4 task = reinterpret_cast<const int4*>(t.wave)[u];
      const bool wide = task.y == -2;
      const int k = wide ? task.x : (row == 0 ? task.x : row == 1 ? task.y : row == 2 ? task.z : task.w);
      const int W = wide ? 64 : 16, j = wide ? lane : (lane & 15);
#pragma unroll
      for (int q = 0; q < N; ++q) s[q] = 0;
      if (k >= 0) br_range_acc(op, t.off[k], t.len[k], j, W, vec, Op::kFlag && t.blk[k] < 0, s);
      // every lane of the wavefront is here.  All N butterflies, then one branch around the N stores: a store per sum in between would
      // cut the butterflies into basic blocks and keep them from overlapping
#pragma unroll
      for (int q = 0; q < N; ++q) s[q] = row_sum(s[q]);
      if (wide) {
#pragma unroll
        for (int q = 0; q < N; ++q) s[q] = rows_to_wave(s[q]);
      }
      if (j == 0 && k >= 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) out[N * (size_t)k + q] = s[q];
      }
    }
    return;
  }
  // ---- large regime: this workgroup reduces one chunk of a block
  const int c = (int)blockIdx.x - nwg_small;
  const int k = t.chunk[2 * (size_t)c];
  const long long first = (long long)t.chunk[2 * (size_t)c + 1] * kBrChunk;
  const long long rest = t.len[k] - first, len = rest < kBrChunk ? rest : kBrChunk;
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = 0;
  br_range_acc(op, t.off[k] + first, len, threadIdx.x, kBrThreads, vec, Op::kFlag && t.blk[k] < 0, s);
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = block_sum(s[q], lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) cpart[N * (size_t)c + q] = s[q];
  }
}

// second stage of the large regime: one wavefront per chunked block adds its chunks, lane l the chunks l, l + 64, ...
template <int N>
__global__ __launch_bounds__(64) void block_reduce_final_kernel(const int* large, const double* cpart, double* out) {
  const int k = large[3 * (size_t)blockIdx.x], first = large[3 * (size_t)blockIdx.x + 1], cnt = large[3 * (size_t)blockIdx.x + 2];
  double s[N];
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = 0;
  for (int c = threadIdx.x; c < cnt; c += 64)
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] += cpart[N * (size_t)(first + c) + q];
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = wave_sum(s[q]);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) out[N * (size_t)k + q] = s[q];
  }
}

// out[N k ..] for every block of the task lists; cpart: N nchunk doubles of scratch.  16-byte loads where every vector is 8-byte aligned
// and all lie in the same 16-byte phase.
template <class Op>
int launch_block_reduce(const Op& op, const BlockTasksView& t, double* cpart, double* out, hipStream_t st) {
  bool ok = out && t.nwave >= 0 && t.nchunk >= 0 && t.nlarge >= 0 && (t.nwave == 0 || t.wave) &&
            (t.nchunk == 0 || (t.chunk && t.large && cpart && t.nlarge >= 1)) && ((t.nwave == 0 && t.nchunk == 0) || (t.off && t.len && (!Op::kFlag || t.blk)));
  bool vec = true;
  for (const double* v : op.p) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(v);
    ok = ok && v;
    vec = vec && (x & 7) == 0 && (x & 15) == (reinterpret_cast<uintptr_t>(op.p[0]) & 15);
  }
  if (!ok) { set_error("%s: invalid argument", Op::kName); return CUADMM_ERR_INVALID; }
  if (t.nwave == 0 && t.nchunk == 0) return CUADMM_OK;
  const int per = kBrThreads / 64;
  const int nwg_small = std::min((t.nwave + per - 1) / per, kBrSmallGrid);
  hipLaunchKernelGGL(block_reduce_kernel<Op>, dim3((unsigned)(nwg_small + t.nchunk)), dim3(kBrThreads), 0, st, op, t, cpart, out, nwg_small, vec ? 1 : 0);
  if (t.nlarge > 0) hipLaunchKernelGGL(block_reduce_final_kernel<Op::N>, dim3((unsigned)t.nlarge), dim3(64), 0, st, t.large, cpart, out);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

// partials[0 .. kBrSlots) <- slot sums of a term over i in [0, n), fixed stride (the slots without work are written as zeros).
// Term: add(s, i), __device__ __forceinline__, adds the term of index i to s.
template <class Term>
__global__ __launch_bounds__(kBrThreads) void slot_partials_kernel(long long n, Term term, double* partials) {
  __shared__ double lds[4];
  double s = 0;
  for (long long i = (long long)blockIdx.x * kBrThreads + threadIdx.x; i < n; i += (long long)kBrSlots * kBrThreads) term.add(s, i);
  s = block_sum(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
template <class Term>
int launch_slot_partials(long long n, const Term& term, double* partials, hipStream_t st) {
  hipLaunchKernelGGL(slot_partials_kernel<Term>, dim3(kBrSlots), dim3(kBrThreads), 0, st, n, term, partials);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}
// The same with N sums per index: partials[q kBrSlots + slot], q < N.  Term: add(s, i) with double (&s)[N]; it may write vectors of
// its own at index i (every index is visited by exactly one thread).
template <int N, class Term>
__global__ __launch_bounds__(kBrThreads) void slot_partials_kernel(long long n, Term term, double* partials) {
  __shared__ double lds[4];
  double s[N];
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = 0;
  for (long long i = (long long)blockIdx.x * kBrThreads + threadIdx.x; i < n; i += (long long)kBrSlots * kBrThreads) term.add(s, i);
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = block_sum(s[q], lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) partials[q * kBrSlots + blockIdx.x] = s[q];
  }
}
template <int N, class Term>
int launch_slot_partials(long long n, const Term& term, double* partials, hipStream_t st) {
  hipLaunchKernelGGL((slot_partials_kernel<N, Term>), dim3(kBrSlots), dim3(kBrThreads), 0, st, n, term, partials);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

}  // namespace cuadmm
