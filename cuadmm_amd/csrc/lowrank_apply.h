// svec(L_k L_k') of a list of blocks, written where the blocks lie in an svec vector (cuadmm_set_lowrank, cuadmm_op_block_outer): the
// task list, the kernel (lowrank_apply.hip) and the device code it shares with lowrank_line.hip.  DESIGN.md, "Starting from low-rank
// factors"; factor_layout.h has the layout of L.
//
// For PSD block k of size n with r = ranks[k] columns every one of its n (n + 1) / 2 slots is written, row by row over the lower triangle:
//   v[off_k + i (i + 1) / 2 + j] = c_ij sum_{t < r} L[i, t] L[j, t],   i >= j,   c_ii = 1,   c_ij = kLoSqrt2 (one rounded constant).
// Columns >= r of L are never read (they may hold NaN), r = 0 writes +0.0, the slots of an unconstrained block keep their bits.
//
// Arithmetic: every size takes the fp64 matrix cores -- 16 x 16 tiles of the lower triangle on v_mfma_f64_16x16x4_f64, K in steps of 4 with
// the lanes of k >= r and of rows >= n feeding 0.0 (selected, not multiplied: what lies there is not loaded); tiles above the diagonal
// are not formed.  The operands come straight from global memory: 16 consecutive rows of a column are one 128-byte segment, and the
// factor (n r numbers) is read again only from the cache.  Each register of the accumulator is one row of 16 consecutive slots.
//
// Rounding, for any order of the sums (u = 2^-53):
//   |computed - exact| <= (r + 4) u c_ij sum_t |L_it| |L_jt|
// -- r products and sums, the multiplication by the constant and the constant's own rounding.  With small-integer L every product and
// sum is exact: the diagonal slots are integers, the others fl(kLoSqrt2 * integer).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace cuadmm {

constexpr double kLoSqrt2 = 1.4142135623730951;
constexpr int kLoTile = 16;
constexpr int kLoWaveMax = 32;            // up to here (<= 3 tiles) one wavefront owns the block, four such blocks share a workgroup
constexpr int kLoSplitFrom = 257;         // from here the tiles of a block are dealt to several workgroups; below, one workgroup owns it
constexpr int kLoRunTiles = 32;           // tiles per workgroup of a split block: 8 per wavefront (n = 2000: 7875 tiles, 247 workgroups)

// What one wavefront does: the tiles t0, t0 + step, ... < t1 of block k, numbered row by row over the lower triangle of tiles
// (tile t = ti (ti + 1) / 2 + tj, tj <= ti).  k < 0: nothing.  A workgroup of 256 reads four consecutive entries.
struct LoTask { int k, t0, t1, step; };

inline int lo_tiles(int n) { const int nt = (n + kLoTile - 1) / kLoTile; return nt * (nt + 1) / 2; }

// The wavefront slots (a multiple of 4) for the PSD blocks of blk; they depend on the block sizes alone.  First the blocks that are split
// (n >= split_from; runs of kLoRunTiles tiles, the four wavefronts of a workgroup interleaved over a run), then the blocks of one
// workgroup each (n > kLoWaveMax), then the small ones, one wavefront each.  loff (may be null): factor_offsets' for this rmax.  Host only.
int lo_build_tasks(int nblk, const int* blk, int rmax, int split_from, std::vector<LoTask>* tasks, std::vector<long long>* loff);

// One launch over nslots wavefront slots (device list).  L, loff, ranks: the factor buffer, its offsets and the columns per block; off,
// blk: first slot and size per block (BlockTasksView's); v: the vector written.  The host has checked 0 <= ranks[k] <= min(n_k, rmax).
int launch_block_outer(int nslots, const LoTask* tasks, const double* L, const long long* loff, const int* ranks, const long long* off, const int* blk,
                       double* v, hipStream_t st);

// Device code of block_outer_kernel and block_outer3_kernel: the row ti of tile = ti (ti + 1) / 2 + tj, tj <= ti -- the root in floating
// point, then at most a step either way.  (By value: handing ti and tj back through references changes an operand order in both kernels.)
__device__ __forceinline__ int lo_tile_row(int tile) {
  int ti = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
  if ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
  if (ti * (ti + 1) / 2 > tile) --ti;
  return ti;
}

}  // namespace cuadmm
