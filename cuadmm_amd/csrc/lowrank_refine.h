// Nonlinear conjugate gradients over per-block factors with everything resident (cuadmm_lowrank_refine, cuadmm_op_lrr_dots,
// cuadmm_op_lrr_direction, cuadmm_op_lrr_step, cuadmm_cg_update): the three streaming launches a step adds to the chains of
// cuadmm_lowrank_grad and cuadmm_lowrank_line (lowrank_refine.hip) and the host-only scalar update (cg_update.cpp).  DESIGN.md, "Refinement
// over factors".
//
// All three walk the `count` doubles of a factor buffer (factor_layout.h) flat: the columns >= r_k hold + 0.0 in L and in the block
// product's W (the engine zeroes W once before the first step; the product never writes there), and zeros stay zeros under b. and c.
// Every operation is rounded once and none is contracted (plain operators under `#pragma clang fp contract(off)`: lowrank_refine.hip).
// W is the block product's output in the engine's units: the gradient in the caller's is G[e] = 2.0 * (W[e] * unit), unit = Cscale,
// the value cuadmm_lowrank_grad returns; it is formed again wherever it is read.
//
// a. lrr_dots: gg = sum G^2, go = sum G G_old, gd = sum G D_old in one read of the three buffers, as 3 x 256 slot partials
//    (launch_slot_partials<3>: fixed stride, no atomics, the same bits on every run; the host adds them with slot_sum).
// b. lrr_direction: D[e] = fl(fl(beta D[e]) - G[e]), or - G[e] on a restart (D is then not read);  Ds[e] = fl(D[e] root), the copy in the
//    units X lies in (root = fl(1 / sqrt(ux)), scale_factors');  G_old[e] = G[e].
// c. lrr_step: L[e] = fl(L[e] + fl(t D[e]));  Ls[e] = fl(L[e] root).
// Where every buffer of a launch is 16-byte aligned a thread takes two entries with one 16-byte load per vector read and one 16-byte
// store per vector written, and the odd last entry alone; otherwise one entry per thread.  The vectors written do not depend on the
// map, the slot sums of a. do.  No LDS beyond the reduce skeleton's, no atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "block_reduce.h"

namespace cuadmm {

constexpr int kRfParts = 3;              // slot sums of lrr_dots: gg, go, gd
constexpr int kRfTrace = 16;             // doubles per step of cuadmm_lowrank_refine's trace

// partials (kRfParts kBrSlots, device) <- the slot sums over n entries of W, G_old, D_old (device)
int launch_lrr_dots(long long n, const double* W, double unit, const double* G_old, const double* D_old, double* partials, hipStream_t st);
// D (read unless restart, written), Ds, G_old (written) over n entries
int launch_lrr_direction(long long n, const double* W, double unit, double beta, int restart, double root, double* D, double* Ds, double* G_old, hipStream_t st);
// L (read and written), Ls (written) over n entries
int launch_lrr_step(long long n, double t, double root, const double* D, double* L, double* Ls, hipStream_t st);

}  // namespace cuadmm
