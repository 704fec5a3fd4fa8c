// The exact quartic of the augmented Lagrangian along a line in factor space (cuadmm_lowrank_line, cuadmm_op_block_outer3,
// cuadmm_op_lrl_sums, cuadmm_quartic_min): the three launches the chain adds to the existing ones (lowrank_line.hip) and the host-only
// minimiser (quartic_min.cpp).  DESIGN.md, "Line search along factor steps".
//
// With x(t) the point whose PSD blocks are (L_k + t D_k)(L_k + t D_k)' (unconstrained slices: the resident ones, for every t):
//   x(t) = x0 + t x1 + t^2 x2,   x0 = L L',  x1 = L D' + D L',  x2 = D D'        r(t) = r0 + t p + t^2 q,   r0 = A x0 - b,  p = A x1,  q = A x2
//   f(t) = <C, x(t)> - y'r(t) + (sigma / 2) ||r(t)||^2 = c0 + c1 t + c2 t^2 + c3 t^3 + c4 t^4.
//
// a. The three outer products in one pass.  The tile decomposition, the task list (LoTask, lo_build_tasks) and the lane layout are those
// of lowrank_apply.hip: one wavefront per 16 x 16 tile of the lower triangle on v_mfma_f64_16x16x4_f64, three accumulators per tile and
// four MFMAs per K-step of 4:
//   acc0 += L_a L_b        acc1 += L_a D_b, then acc1 += D_a L_b        acc2 += D_a D_b
// Lanes of k >= r or of rows >= n feed 0.0 (selected: what lies there is not loaded).  Every slot of a PSD block is written in each of
// x0, x1, x2 (the diagonal as it is, the others times kLoSqrt2 once); the slots of an unconstrained block keep their bits in all three.
// acc0 and acc2 each run the instruction sequence of block_outer_kernel: x0 and x2 are bit for bit what that kernel writes from L and
// from D.  Negating D negates every product that enters acc1 and none that enters acc0 or acc2: x1 changes sign bit for bit.
// Rounding (u = 2^-53): x0 and x2 as in lowrank_apply.h, (r + 4) u c_ij sum_t |L_it| |L_jt|;
//   x1: |computed - exact| <= (2 r + 4) u c_ij sum_t (|L_it| |D_jt| + |D_it| |L_jt|)
// -- 2 r products and sums, the multiplication by the constant and the constant's own rounding.  No LDS, no barrier, no atomics.
//
// b. The quartic sums, one streaming pass over the m constraints in the engine's permuted, scaled space (the shape of lrg_multiplier,
// lowrank_grad.hip).  With ax_j = A x_j as the SpMV left them, b and y scaled, every operation rounded once and none contracted:
//   rs0_i = xunit ax0_i - b_i      r0_i = (normA_i rs0_i) bscale          (lrg_multiplier's rs and r: the same bits)
//   ps_i  = xunit ax1_i            p_i  = (normA_i ps_i) bscale           qs_i, q_i likewise from ax2
//   partials[256 j .. 256 j + 256), j = 0 .. 8: slot sums of  y rs0, y ps, y qs  (times bscale Cscale: the caller's units),
//                                               r0^2, r0 p, p^2, r0 q, p q, q^2
// Where the nine vectors are 16-byte aligned a thread takes two constraints with one 16-byte load per vector and one 16-byte store per
// output, and the odd last constraint alone; otherwise one constraint per thread.  launch_slot_partials<9>: fixed stride, no atomics, the
// same bits on every run.
//
// c. The per-block objective terms, one Op on block_reduce.h's skeleton over C, x0, x1, x2: sum C_i x0_i, sum C_i x1_i, sum C_i x2_i per
// block (on an unconstrained block x1 and x2 are zero and x0 is the resident slice).
//
// The coefficients are formed on the host in plain doubles, nothing contracted, in this order (S_j: a kernel's 256 slot partials added in
// slot order from 0.0; cx_j: the blocks' (sum C x_j)(Cscale ux) added in block order from 0.0; yr_j = S_j (bscale Cscale); h = 0.5 sigma):
//   c0 = (cx_0 - yr_0) + h S_3
//   c1 = (cx_1 - yr_1) + sigma S_4
//   c2 = (cx_2 - yr_2) + h (S_5 + 2 S_6)
//   c3 = sigma S_7
//   c4 = h S_8
// c0 is formed as cuadmm_lowrank_grad forms f.  Negating D negates S_1, S_4, S_7 and cx_1 bit for bit and leaves the others.
#pragma once
#include <hip/hip_runtime.h>

#include "block_reduce.h"
#include "lowrank_apply.h"

namespace cuadmm {

constexpr int kLlSums = 3;               // per block: sum C x0, sum C x1, sum C x2
constexpr int kLlParts = 9;              // slot sums of the streaming pass

// One launch over nslots wavefront slots (device list, lo_build_tasks').  L, D: two factor buffers of one layout (loff, ranks); off, blk:
// first slot and size per block; x0, x1, x2: the vectors written.  The host has checked 0 <= ranks[k] <= min(n_k, rmax).
int launch_block_outer3(int nslots, const LoTask* tasks, const double* L, const double* D, const long long* loff, const int* ranks, const long long* off,
                        const int* blk, double* x0, double* x1, double* x2, hipStream_t st);

// r0, p, q (m doubles each, device) and partials (kLlParts kBrSlots) as above.
int launch_lrl_sums(int m, const double* ax0, const double* ax1, const double* ax2, const double* b, const double* normA, const double* y, double xunit,
                    double bscale, double* r0, double* p, double* q, double* partials, hipStream_t st);

// sums[3k ..] for every block of the task lists; cpart: kLlSums nchunk doubles of scratch
int launch_lrl_block_terms(const double* C, const double* x0, const double* x1, const double* x2, const BlockTasksView& t, double* cpart, double* sums,
                           hipStream_t st);

}  // namespace cuadmm
