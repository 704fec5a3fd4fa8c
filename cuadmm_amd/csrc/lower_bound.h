// Certified dual lower bound from trace bounds (cuadmm_lower_bound, option "gap_check"): the per-block norms and the combine kernel
// (lower_bound.hip; the reduction itself is block_reduce.h's) and the trace-bound detection on the problem's arrays.  DESIGN.md, "Certified lower bound".
#pragma once
#include <hip/hip_runtime.h>

#include "block_reduce.h"

namespace cuadmm {

// Accuracy of the projection kernels as their tests state it (tests/test_gpu_psd_plan_state.py): every entry of a projected block
// within 2e-12 sqrt(2) ||M_k||_2 of the exact projection, so ||P_k - P+(M_k)||_F <= kLbProjErr sqrt(len_k) ||M_k||_F (the spectral
// norm is not available without an eigenvalue: the Frobenius norm stands in for it).
constexpr double kLbProjErr = 2e-12 * 1.4142135623730951;

// pairs[2k] = ||M_k||^2, pairs[2k + 1] = ||P_k||^2 for every block of the task lists (block_reduce.h: one pass over M and P, no atomics,
// the same bits every run); cpart: 2 nchunk doubles of scratch
int launch_lb_block_norms(const double* M, const double* P, const BlockTasksView& t, double* cpart, double* pairs, hipStream_t st);

// partials[0 .. kBrSlots) <- slot sums of a[i] b[i] (fixed stride; the slots without work are written as zeros)
int launch_lb_dot(long long n, const double* a, const double* b, double* partials, hipStream_t st);

// out4 = [sum_k R_k nubar_k, worst block, its term R_k nubar_k, sum of the dot partials]; nubar_k = sqrt(pairs[2k+1]) +
// (blk[k] >= 0 ? kLbProjErr sqrt(len_k) sqrt(pairs[2k]) : 0).  One workgroup, fixed order.  dot_partials may be null (then out4[3] = 0).
int launch_lb_combine(int nblk, const double* pairs, const double* R, const long long* len, const int* blk, const double* dot_partials,
                      double* out4, hipStream_t st);

// Trace bounds read off the constraints (host only; cuadmm_trace_bounds_detect in the public header has the rules).
int lb_trace_bounds_detect(int vec_len, int con_num, const int* At_cp, const int* At_ri, const double* At_vx, const int* b_idx,
                           const double* b_val, int b_nnz, const int* blk, int mat_num, double* R_out);

}  // namespace cuadmm
