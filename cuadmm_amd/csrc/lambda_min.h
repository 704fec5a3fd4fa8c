// Certified per-block lower bounds on lambda_min by shifted-Cholesky bisection (cuadmm_lambda_min, cuadmm_op_block_lambda_min):
// the size classes, the batched kernel (lambda_min.hip) and the margin of a successful trial.  DESIGN.md, "Certified lambda_min".
//
// A trial is the floating-point Cholesky factorisation of M + mu I.  Where it runs to completion, lambda_min(M) >= -mu - margin(n, tr M, mu)
// is a theorem about IEEE arithmetic (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3); where it breaks down nothing is
// claimed.  So `lo` is certified and `hi`, the largest shift that failed, is an estimate only.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace cuadmm {

constexpr int kLmOut = 4;                 // per block: lo, hi, flag, ||M_k||_F (PSD block) or ||v_k||_2 (unconstrained)
constexpr int kLmSmall = 32;              // up to here one wavefront owns the block; beyond, a workgroup of 256
constexpr int kLmLds = 200;               // n_lds: the packed scratch triangle, n (n + 1) / 2 doubles, fits the 160 KiB of one workgroup up to here
constexpr int kLmMax = 1024;              // largest block that is refined (scratch in the global workspace beyond kLmLds)
constexpr int kLmStepsMax = 40;
constexpr double kLmRangeLo = 0x1p-500, kLmRangeHi = 0x1p500;      // max |m_ij| outside: the analysis would have to deal with under- / overflow

enum { kLmRefined = 0, kLmPsdAtFloor = 1, kLmFree = 2, kLmUnrefined = 3 };

// (n + 2) 2^-52 (trace + n mu): twice what the theorem needs, DESIGN.md has the derivation.  Host and device use this one expression.
__host__ __device__ inline double lm_margin(int n, double trace, double mu) { return ((double)(n + 2) * 0x1p-52) * (trace + (double)n * mu); }

// The blocks of one launch: those of a size class, each owned by one workgroup.
struct LmClass {
  std::vector<int> blocks;                // indices into the blk array
  std::vector<long long> work;            // first double of the block's scratch in the global workspace (class of kLmMax only)
  int nmax = 0;                           // largest size in the class: sizes the dynamic LDS
};
// classes by size: <= 32, <= 64, <= 128, <= kLmLds (scratch in LDS), <= kLmMax (scratch in the workspace), and the rest (no trial:
// unconstrained blocks and blocks beyond kLmMax).  *work_doubles: the workspace the fifth class needs.
constexpr int kLmClasses = 6;
int lm_build_classes(int nblk, const int* blk, LmClass (&cls)[kLmClasses], long long* work_doubles);

// One launch: out[kLmOut k ..] for every block k of `list` (device, count entries).  v: the svec vector, read as sign * v (sign = +-1,
// exact); off, blk: first slot and size per block (BlockTasksView's).  cls: which class the list is (0 .. kLmClasses - 1); nmax: its
// largest size; work / work_off: the global workspace and the blocks' offsets into it (class 4 only).
int launch_lambda_min(int cls, int count, int nmax, const int* list, const double* v, double sign, const long long* off, const int* blk, int steps,
                      double* work, const long long* work_off, double* out, hipStream_t st);

}  // namespace cuadmm
