// Certified dual lower bound from trace bounds (cuadmm_lower_bound, option "gap_check"): the per-block norm kernels (lower_bound.hip),
// the task lists they walk and the trace-bound detection on the problem's arrays.  DESIGN.md, "Certified lower bound".
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace cuadmm {

constexpr int kLbThreads = 256;
constexpr long long kLbRowMax = 128;     // a block of up to this many slots is owned by 16 lanes (one DPP row), four blocks per wavefront
constexpr long long kLbChunk = 8192;     // a block of up to this many slots is owned by one wavefront; a longer one is cut into chunks of
                                         // this length (even: a chunk starts in the 16-byte phase of its block), one workgroup each
constexpr int kLbSmallGrid = 2048;       // workgroups of the small regime at most (a wavefront strides over its tasks: whole blocks,
                                         // so the sums do not depend on the grid)
constexpr int kLbDotSlots = 256;         // workgroups = partial sums of b'y
// Accuracy of the projection kernels as their tests state it (tests/test_gpu_psd_plan_state.py): every entry of a projected block
// within 2e-12 sqrt(2) ||M_k||_2 of the exact projection, so ||P_k - P+(M_k)||_F <= kLbProjErr sqrt(len_k) ||M_k||_F (the spectral
// norm is not available without an eigenvalue: the Frobenius norm stands in for it).
constexpr double kLbProjErr = 2e-12 * 1.4142135623730951;

// What the norm kernel walks, built on the host from the blocks' lengths.
struct LbTasks {
  std::vector<int> wave;    // 4 per wavefront task: the blocks of its four 16-lane rows (-1: none), or {k, -2, -2, -2}: the wavefront owns block k
  std::vector<int> chunk;   // 2 per workgroup task: block, chunk index
  std::vector<int> large;   // 3 per chunked block: block, first workgroup task, chunks
  int nwave() const { return (int)(wave.size() / 4); }
  int nchunk() const { return (int)(chunk.size() / 2); }
  int nlarge() const { return (int)(large.size() / 3); }
};
int lb_build_tasks(int nblk, const long long* len, LbTasks* out);

struct LbNormArgs {
  const double *M, *P;              // the two vectors; 16-byte loads where both have the same 16-byte phase
  const long long *off, *len;       // per block: first slot and slots (device)
  const int *wave, *chunk, *large;  // LbTasks on the device
  int nwave, nchunk, nlarge;
  double* cpart;                    // 2 nchunk doubles of scratch
  double* pairs;                    // out, 2 per block: ||M_k||^2, ||P_k||^2
};
// pairs[2k], pairs[2k + 1] for every block of the task lists; one pass over M and P, no atomics, the same bits every run
int launch_lb_block_norms(const LbNormArgs& a, hipStream_t st);

// partials[0 .. kLbDotSlots) <- slot sums of a[i] b[i] (fixed stride; the slots without work are written as zeros)
int launch_lb_dot(long long n, const double* a, const double* b, double* partials, hipStream_t st);

// out4 = [sum_k R_k nubar_k, worst block, its term R_k nubar_k, sum of the dot partials]; nubar_k = sqrt(pairs[2k+1]) +
// (blk[k] >= 0 ? kLbProjErr sqrt(len_k) sqrt(pairs[2k]) : 0).  One workgroup, fixed order.  dot_partials may be null (then out4[3] = 0).
int launch_lb_combine(int nblk, const double* pairs, const double* R, const long long* len, const int* blk, const double* dot_partials,
                      double* out4, hipStream_t st);

// Trace bounds read off the constraints (host only; cuadmm_trace_bounds_detect in the public header has the rules).
int lb_trace_bounds_detect(int vec_len, int con_num, const int* At_cp, const int* At_ri, const double* At_vx, const int* b_idx,
                           const double* b_val, int b_nnz, const int* blk, int mat_num, double* R_out);

}  // namespace cuadmm
