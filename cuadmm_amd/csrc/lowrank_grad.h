// Value and gradient of the augmented Lagrangian at per-block factors (cuadmm_lowrank_grad, cuadmm_op_lrg_multiplier): the two launches
// the chain adds to the existing ones (lowrank_grad.hip).  DESIGN.md, "Value and gradient at factors".
//
// The multiplier pass, one streaming kernel over the m constraints in the engine's permuted, scaled space.  With ax = A x as the SpMV left
// it (xunit ax in the scaled units: xunit = 1 where x is scaled, 1 / bscale where it is in the caller's units), b and y scaled,
// ics = fl(1 / Cscale), every operation rounded once and none contracted:
//   rs_i     = xunit ax_i - b_i                       the scaled residual
//   r_i      = (normA_i rs_i) bscale                  r = A x - b in the caller's units (the iteration's ||Rp|| is the norm of this)
//   ytilde_i = y_i - ((sigma r_i) normA_i) ics        the scaled y - sigma r, as stage_scaled_y scales a caller's y; sigma == 0: y_i's bits
//   partials[0 .. 256)   slot sums of y_i rs_i        (times bscale Cscale: y'r in the caller's units)
//   partials[256 .. 512) slot sums of r_i^2
// Where the six vectors are 16-byte aligned a thread takes two constraints with one 16-byte load per vector and one 16-byte store per
// output, and the odd last constraint alone; otherwise one constraint per thread.  The slot sums are launch_slot_partials': fixed
// stride, no atomics, the same bits on every run (they differ between the two element-to-thread maps, the vectors written do not).
//
// The per-block terms, one Op on block_reduce.h's skeleton over C, x and M = A'ytilde - C (all scaled): sum C_i x_i for every block and
// sum M_i^2 for an unconstrained one (a PSD block gets 0 there: its ||G_k||_F is a host sum over the returned G).
#pragma once
#include <hip/hip_runtime.h>

#include "block_reduce.h"

namespace cuadmm {

constexpr int kLgSums = 2;               // per block: sum C x, sum M^2 (unconstrained blocks only)

// ytilde, r (m doubles each, device) and partials (2 kBrSlots) as above.  ytilde may not alias y.
int launch_lrg_multiplier(int m, const double* ax, const double* b, const double* normA, const double* y, double xunit, double bscale, double ics, double sigma,
                          double* ytilde, double* r, double* partials, hipStream_t st);

// sums[2k ..] for every block of the task lists; cpart: kLgSums nchunk doubles of scratch
int launch_lrg_block_terms(const double* C, const double* x, const double* M, const BlockTasksView& t, double* cpart, double* sums, hipStream_t st);

}  // namespace cuadmm
