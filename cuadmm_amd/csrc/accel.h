// Safeguarded Anderson acceleration of the iteration (option "accel"): launchers of the three stream kernels (accel.hip) and the
// host solve of the small least-squares system.  DESIGN.md, "Acceleration".
//
// Vectors of the accelerated state have two halves, the X part and the S part, `hs` doubles apart (hs >= L; the engine rounds L up
// to an even number so that both halves start on a 16-byte boundary).  The state vectors u, f hold X and S as they are; sigma enters
// where differences are formed: g = (X - u_X, sigma (S - u_S)), so the rings hold columns in the units of u = (X, sigma S).
#pragma once
#include <hip/hip_runtime.h>

namespace cuadmm {

constexpr int kAccelMaxMem = 16;      // most columns of the rings (option "accel": its row in option_table.h spells this bound, kOptAccelMaxMem and the refusal text)
constexpr int kAccelSlots = 1024;     // workgroups of the reductions = partial sums per dot product (fixed: the sums do not depend on the device)
constexpr int kAccelThreads = 256;

// doubles of scratch the reductions need (partials) / produce (dots: 2 * kAccelMaxMem dots + ||g||^2)
constexpr size_t kAccelPartials = (size_t)kAccelSlots * (2 * kAccelMaxMem);
constexpr int kAccelDots = 2 * kAccelMaxMem + 1;

// One pass over u (the state the iteration started from), X, S (what it produced): g_out = (X - u_X, sig (S - u_S)); with have_prev
// the ring columns dF_out = (X - f_prev_X, sig (S - f_prev_S)) and dG_out = g - g_prev; f_out = (X, S); gnorm2_out[0] = ||g||^2.
// u, f_prev, f_out may be the same buffer, g_prev and g_out too (every element is read before it is written, by one thread).
int launch_aa_push(long long L, long long hs, const double* u, const double* X, const double* S, double sig, const double* f_prev, const double* g_prev,
                   int have_prev, double* g_out, double* f_out, double* dF_out, double* dG_out, double* partials, double* gnorm2_out, hipStream_t st);

// dots[j] = <dG_newest, dG_j>, dots[cols + j] = <dG_j, g> for the columns j < cols of the ring (column j at ring_dG + j * col_stride);
// n = elements per column that count (both halves: the X part [0, L) and the S part [hs, hs + L)).
int launch_aa_gram(long long L, long long hs, long long col_stride, int cols, int newest, const double* ring_dG, const double* g, double* partials,
                   double* dots, hipStream_t st);

// X <- X - sum_j gamma_j dF_j[X], S <- (sig S - sum_j gamma_j dF_j[S]) / sig, the sums carried in double-double; u_out (optional)
// receives the new (X, S).
int launch_aa_combine(long long L, long long hs, long long col_stride, int cols, const double* ring_dF, const double* gamma, double sig, double* X,
                      double* S, double* u_out, hipStream_t st);

// (G + reg tr(G) / cols I) gamma = rhs by Cholesky in long double; CUADMM_ERR_FACTOR when a pivot is not positive.  Host only.
int accel_solve_ls(const double* gram, const double* rhs, int cols, double reg, double* gamma_out);

}  // namespace cuadmm
