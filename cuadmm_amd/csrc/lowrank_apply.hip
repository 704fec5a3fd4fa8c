// svec(L_k L_k') per block on the fp64 matrix cores, written into an svec vector where the blocks lie: lowrank_apply.h has the task
// list and the rounding contract, factor_layout.h the layout of L, DESIGN.md, "Starting from low-rank factors", the sizes and what
// was measured.
//
// One wavefront forms one 16 x 16 tile at a time.  v_mfma_f64_16x16x4_f64: lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
// and holds D[row = (l >> 4) + 4 reg][col = l & 15], so a register is four rows of 16 consecutive svec slots (128 bytes each).  No LDS,
// no barrier, nothing waits on another wavefront; the loops are bounded by the task's tile range and by r.
#include <hip/hip_runtime.h>

#include "lowrank_apply.h"
#include "factor_layout.h"
#include "device_util.h"

namespace cuadmm {
namespace {

typedef double lo_v4f64 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void block_outer_kernel(const LoTask* __restrict__ tasks, const double* __restrict__ L, const long long* __restrict__ loff,
                                                          const int* __restrict__ ranks, const long long* __restrict__ off, const int* __restrict__ blk,
                                                          double* __restrict__ v) {
  const int lane = (int)threadIdx.x & 63;
  const LoTask t = tasks[blockIdx.x * 4 + ((int)threadIdx.x >> 6)];
  if (t.k < 0) return;
  const int n = blk[t.k], r = ranks[t.k];
  if (n <= 0) return;                        // (the host lists PSD blocks only)
  const double* Lk = L + loff[t.k];          // column c at Lk + c n
  double* x = v + off[t.k];
  const int r16 = lane & 15, kk = lane >> 4;
  for (int tile = t.t0; tile < t.t1; tile += t.step) {
    const int ti = lo_tile_row(tile), tj = tile - ti * (ti + 1) / 2;
    const int ia = kLoTile * ti + r16, ib = kLoTile * tj + r16;
    lo_v4f64 acc = lo_v4f64{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < r; k0 += 4) {      // wave-uniform trip count
      const int k = k0 + kk;
      const double a = (k < r && ia < n) ? Lk[(size_t)k * n + ia] : 0.0;
      const double b = (k < r && ib < n) ? Lk[(size_t)k * n + ib] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    const int col = ib;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = kLoTile * ti + kk + 4 * q;
      if (row < n && col <= row) x[(long long)row * (row + 1) / 2 + col] = col == row ? acc[q] : acc[q] * kLoSqrt2;
    }
  }
}

}  // namespace

int lo_build_tasks(int nblk, const int* blk, int rmax, int split_from, std::vector<LoTask>* tasks, std::vector<long long>* loff) {
  std::vector<long long> own;
  if (split_from <= kLoWaveMax || !tasks) { set_error("block_outer: invalid argument"); return CUADMM_ERR_INVALID; }
  int rc = factor_offsets("block_outer", nblk, blk, rmax, loff ? loff : &own);
  if (rc) return rc;
  tasks->clear();
  auto team = [&](int k, int t0, int t1) {   // one workgroup: its four wavefronts interleaved over [t0, t1)
    for (int w = 0; w < 4; ++w) tasks->push_back(LoTask{k, t0 + w, t1, 4});
  };
  for (int k = 0; k < nblk; ++k)
    if (blk[k] >= split_from)
      for (int t0 = 0, T = lo_tiles(blk[k]); t0 < T; t0 += kLoRunTiles) team(k, t0, t0 + kLoRunTiles < T ? t0 + kLoRunTiles : T);
  for (int k = 0; k < nblk; ++k)
    if (blk[k] > kLoWaveMax && blk[k] < split_from) team(k, 0, lo_tiles(blk[k]));
  for (int k = 0; k < nblk; ++k)
    if (blk[k] > 0 && blk[k] <= kLoWaveMax) tasks->push_back(LoTask{k, 0, lo_tiles(blk[k]), 1});
  while (tasks->size() % 4) tasks->push_back(LoTask{-1, 0, 0, 1});
  return CUADMM_OK;
}

int launch_block_outer(int nslots, const LoTask* tasks, const double* L, const long long* loff, const int* ranks, const long long* off, const int* blk,
                       double* v, hipStream_t st) {
  if (nslots < 0 || nslots % 4 || (nslots > 0 && (!tasks || !L || !loff || !ranks || !off || !blk || !v))) {
    set_error("block_outer: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  if (nslots == 0) return CUADMM_OK;
  hipLaunchKernelGGL(block_outer_kernel, dim3((unsigned)(nslots / 4)), dim3(256), 0, st, tasks, L, loff, ranks, off, blk, v);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

}  // namespace cuadmm
