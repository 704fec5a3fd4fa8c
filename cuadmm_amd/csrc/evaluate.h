// KKT and DIMACS report of any point (X, y, S) (cuadmm_evaluate): the streaming per-block statistics (block_reduce.h's skeleton with
// five vectors and six sums) and the small reductions behind them (evaluate.hip).  DESIGN.md, "Evaluation of a point".
#pragma once
#include <hip/hip_runtime.h>

#include "block_reduce.h"

namespace cuadmm {

constexpr int kEvSums = 6;               // per block: sum X^2, sum (PX - X)^2, sum S^2, sum (PS - S)^2, sum X S, sum (Rd1 + S)^2
constexpr int kEvGlobals = 8;            // ev_combine: [sum vX_k^2, sum vS_k^2, <X, S>, sum Rd^2, <C, X>, b'y, sum (normA (A X - b) bscale)^2, unused]

// sums[6k ..] for every block of the task lists: one pass over the five vectors, Rd = Rd1 + S formed in flight.  With P = P+(.) the
// second and fourth sums are ||P+(-X_k)||^2 and ||P+(-S_k)||^2 (P+(M) - M = P+(-M)); an unconstrained block (t.blk[k] < 0: primal cone
// everything, dual cone {0}) gets 0 and sum S^2 there.  cpart: kEvSums nchunk doubles of scratch.
int launch_ev_block_stats(const double* X, const double* S, const double* PX, const double* PS, const double* Rd1, const BlockTasksView& t,
                          double* cpart, double* sums, hipStream_t st);

// partials[0 .. kBrSlots) <- slot sums of (normA[i] (b[i] - ax[i]) bscale)^2: ||A X - b||^2 in the caller's units (fixed stride)
int launch_ev_rp(int m, const double* ax, const double* b, const double* normA, double bscale, double* partials, hipStream_t st);

// out8 (kEvGlobals) from the per-block sums and the three arrays of kBrSlots partials (<C, X>, b'y, ev_rp); one workgroup, fixed order
int launch_ev_combine(int nblk, const double* sums, const double* cx_part, const double* by_part, const double* rp_part, double* out8, hipStream_t st);

}  // namespace cuadmm
