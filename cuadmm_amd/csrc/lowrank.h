// Per-block numerical rank and low-rank factor by Cholesky with diagonal pivoting (cuadmm_lowrank, cuadmm_op_block_lowrank): the size
// classes, the layout of the factor buffer and the batched kernel (lowrank.hip).  DESIGN.md, "Low-rank factors".
//
// For a block M of size n, a relative tolerance tol and a column cap rc = min(n, rmax) the kernel takes pivots p_0, p_1, ... by the largest
// residual diagonal entry (ties: the smallest index) while that entry exceeds thr = tol max(max_i m_ii, 0), in the lazy left-looking form:
// column r is m_{. p} minus the r products of the columns before it, so the Schur complement is never formed and the scratch is O(n r).
// With E = M - L L', d the residual diagonal where it stopped and u = 2^-53 the factor promises
//   structure          L[piv[j], j] > 0, L[piv[i], j] == 0.0 exactly for i < j, columns >= rank are zero;
//   residual diagonal  |E_ii - d_i| <= 2 (r + 2) u (m_ii + sum_j L_ij^2) for every row (d_i = 0 for the pivot rows);
//   PSD input          ||M - L L'||_F <= resid + 4 (n + 2) u tr M;
//   rank               max_i d_i >= tr E / n >= lambda_{r+1}(M) / n after r columns: a matrix of exact rank r0 with
//                      lambda_{r0}(M) / n > tol max_i m_ii is reported with rank r0.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace cuadmm {

constexpr int kLrOut = 6;                 // per block: rank, resid, dneg, trace, flag, offset of its L in the factor buffer
constexpr int kLrSmall = 32;              // up to here one wavefront owns the block; beyond, a workgroup of 256
constexpr double kLrRangeLo = 0x1p-500, kLrRangeHi = 0x1p500;      // lambda_min.h's range, for its reason: the statements above assume no under- / overflow

enum { kLrComplete = 0, kLrCapped = 1, kLrFree = 2, kLrNotFactored = 3 };

// The blocks of one launch: those of a size class, each owned by one workgroup.
struct LrClass {
  std::vector<int> blocks;                // indices into the blk array
  int nmax = 0;                           // largest size in the class: with rmax it sizes the dynamic LDS
};
// classes by size: <= 32 together with the unconstrained blocks (one wavefront), <= 128, <= 1024, the rest (a workgroup of 256 each; they
// differ in the LDS a workgroup asks for, which sets how many share a CU).  loff: factor_offsets' (factor_layout.h); poff[k]: first int of
// block k's factor_cols pivots in the device's pivot buffer, which is kept dense (the caller's pivot array uses the factor's offsets).
// nblk + 1 entries each.
constexpr int kLrClasses = 4;
int lr_build_classes(int nblk, const int* blk, int rmax, LrClass (&cls)[kLrClasses], std::vector<long long>* loff, std::vector<long long>* poff);

// One launch: out[kLrOut k ..], Lbuf[loff[k] ..] and piv[poff[k] ..] for every block k of `list` (device, count entries), every entry of
// the three written.  v: the svec vector, read as sign * v (sign = +-1, exact); off, blk: first slot and size per block (BlockTasksView's).
// cls: which class the list is; nmax: its largest size.
int launch_lowrank(int cls, int count, int nmax, const int* list, const double* v, double sign, const long long* off, const int* blk, double tol, int rmax,
                   const long long* loff, const long long* poff, double* Lbuf, int* piv, double* out, hipStream_t st);

}  // namespace cuadmm
