// W_k = M_k V_k for a list of blocks held as svec (cuadmm_block_multiply, cuadmm_op_block_mult): the task list and the kernel
// (block_mult.hip).  DESIGN.md, "Blocks times factors"; factor_layout.h has the layout of V and W.
//
// For PSD block k of size n, first slot off_k, with r = ranks[k] columns of V_k:
//   offd_it = sum_{j != i} s_ij V[j, t],   s_ij = v[off_k + max(i, j) (max(i, j) + 1) / 2 + min(i, j)]   (the raw svec slots)
//   W[i, t] = sign * fma(kInvSqrt2, offd_it, s_ii * V[i, t])
// The off-diagonal slots enter the sum as they lie; the 1 / sqrt(2) they carry is taken out once per output by that fma (n r scalings
// instead of n^2), with the projection kernels' rounded constant (psd_device.h: kSqrt2Inv, the same double).  Unconstrained blocks are not read.
// Columns >= r of V are never read (they may hold NaN) and the kernel writes nothing there (r = 0: nothing at all): the host puts + 0.0
// into those entries of W.
//
// Arithmetic: every size takes the fp64 matrix cores.  One wavefront owns a panel of 16 rows of W and walks K = n in steps of 4 on
// v_mfma_f64_16x16x4_f64: the part j < i of its rows is read along the packed rows, the part j > i from the rows below (the transposed
// slots, 16 consecutive doubles per k), the diagonal lanes and the lanes of rows >= n, of k >= n and of columns >= r feed 0.0 (selected:
// nothing is loaded there).  Up to four column groups of 16 (r <= 64) are accumulated at once; beyond that the panel is walked again.
// The operands come straight from global memory: every off-diagonal slot is read twice in all (by the panel of its row and by the panel
// of its column), every diagonal slot once.  A row of W has one owner: no atomics, nothing waits on another wavefront, the same bits on
// every run.
//
// Rounding, for any order of the sums (u = 2^-53, M_ij the exact entry s_ij / sqrt(2) or s_ii):
//   |W[i, t] - exact| <= (n + 4) u sum_j |M_ij| |V[j, t]|
// -- n products and sums, the scaling, the constant's own rounding and one spare.  With small-integer slots and V every product and sum
// is exact and the result is sign * RN(kInvSqrt2 * offd + s_ii V_it), the correctly rounded value of an exact rational.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace cuadmm {

constexpr double kInvSqrt2 = 0.7071067811865476;      // = kSqrt2Inv of the projection kernels' svec -> dense load
constexpr int kBmPanel = 16;              // rows of W per wavefront
constexpr int kBmGroups = 4;              // column groups of 16 accumulated at once

// What one wavefront does: panel p (rows 16 p ..) of block k.  k < 0: nothing.  A workgroup of 256 reads four consecutive entries.
struct BmTask { int k, p; };

inline int bm_panels(int n) { return (n + kBmPanel - 1) / kBmPanel; }

// The wavefront slots (a multiple of 4) for the PSD blocks of blk; they depend on the block sizes alone.  First the blocks of several
// panels, the largest first, each padded to whole workgroups (a workgroup holds panels of one block), then the blocks of one panel, four
// to a workgroup.  loff (may be null): factor_offsets' for this rmax.  Host only.
int bm_build_tasks(int nblk, const int* blk, int rmax, std::vector<BmTask>* tasks, std::vector<long long>* loff);

// One launch over nslots wavefront slots (device list).  v: the svec vector read; V, W, loff, ranks: the two factor buffers, their
// offsets and the columns per block; off, blk: first slot and size per block (BlockTasksView's).  The host has checked
// 0 <= ranks[k] <= min(n_k, rmax).
int launch_block_mult(int nslots, const BmTask* tasks, const double* v, double sign, const double* V, double* W, const long long* loff, const int* ranks,
                      const long long* off, const int* blk, hipStream_t st);

}  // namespace cuadmm
