/*
 * cuadmm_amd.h -- C ABI of the MI355X-native SDP-ADMM iteration engine.
 *
 * Drop-in boundary for the hot path of ComputationalRobotics/cuADMM: the class
 * SDPSolver (reference include/cuadmm/solver.h:30-248, src/solver.cu) as driven by its two
 * front ends (src/main.cu:22-41, MATLAB/cuadmm_MATLAB.cu:342-424).  The reference has no
 * FFI layer; a maintainer binds these entry points where the reference constructs and
 * calls SDPSolver.  Plain pointers and sizes only; all indices are
 * 0-based int32 as in the reference; all vectors fp64.
 *
 * Every function returns CUADMM_OK (0) or a negative error code; cuadmm_last_error()
 * returns a human readable message for the calling thread.  Nothing here falls back to a
 * CPU implementation of the device path: without a usable gfx950 device the compute entry
 * points fail with CUADMM_ERR_NO_DEVICE.
 */
#ifndef CUADMM_AMD_H
#define CUADMM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUADMM_OK 0
#define CUADMM_ERR_INVALID (-1)    /* bad argument / bad state                          */
#define CUADMM_ERR_NO_DEVICE (-2)  /* no HIP device, or a HIP call failed               */
#define CUADMM_ERR_IO (-3)         /* unreadable / malformed input file                 */
#define CUADMM_ERR_FACTOR (-4)     /* A A^T factorisation failed                        */
#define CUADMM_ERR_EIG (-5)        /* an eigen-iteration hit its iteration cap          */
#define CUADMM_ERR_COMM (-6)       /* collective hook failed                            */
#define CUADMM_ERR_ALLOC (-7)      /* out of host memory (std::bad_alloc caught at the boundary) */
#define CUADMM_ERR_INTERNAL (-8)   /* a C++ exception other than bad_alloc reached the boundary  */

const char* cuadmm_last_error(void);
const char* cuadmm_version(void);
/* number of visible HIP devices (0 if none); never initialises a device context */
int cuadmm_device_count(void);

/* ------------------------------------------------------------------------------------ */
/* Solver object: replaces `SDPSolver solver;` (reference src/main.cu:21).               */
/* ------------------------------------------------------------------------------------ */
typedef struct cuadmm_solver cuadmm_solver;

int cuadmm_create(cuadmm_solver** out);
void cuadmm_destroy(cuadmm_solver* s);

/* Engine options; call before cuadmm_init.  Unknown keys -> CUADMM_ERR_INVALID; so are a value that is not finite and, for a key that takes an
 * integer (every key but eig_rank_maxfeas, batch_mixed, accel_safeguard, accel_reg, infeas_tol, gap_tol), a value beyond the range of int.
 * Integer keys truncate toward zero.  The keys below are in the order of the option tables (csrc/option_table.h, csrc/psd_options.h: the one
 * place where keys, defaults, environment variables and checks are written down; cuadmm_option_info lists them).
 *   "device"        HIP device ordinal (default 0; the reference hard-wires GPU0, utils.h:4)
 *   "verbose"       1 = print the reference's census + iteration table to stdout (default 1)
 *   "rank","world"  shard blocks by index over `world` engines (default 0,1); see
 *                   cuadmm_set_allreduce
 *   "profile"       default 0; 1 = time every kernel class with HIP events on the engine stream;
 *                   2 = time only the dominant kernel (psd_project)
 *   "force_comm"    default 0; 1 = call the collective hook even when world == 1 (transport tests on one GPU)
 *   "eig_rank"      default 0; r > 0: rank-limited projection (only the r largest eigenvalues of every PSD block survive; reference
 *                   dense_scalar.cu:51-57 + get_eig_rank_mask.cu, dormant there); active from iteration
 *                   "eig_rank_begin_iter" (default 0) on, or once maxfeas < "eig_rank_maxfeas" (default 0 = never);
 *                   set before cuadmm_init (every block then takes the eigensolver kernels)
 *   "psd_steps"     default 0; 1 = record how many Newton-Schulz steps the adaptive matrix-sign projection took per block
 *                   (cuadmm_get_psd_steps); set before cuadmm_init
 *   "duo_share_device", "duo_exchange"   the in-process group of cuadmm_duo_init(device_num_requested = N): all engines on the
 *                   caller's device (1; default 0); all-reduce through device memory (1), host staging (0), chosen by peer accessibility (-1, default)
 *   "accel"         memory m of the safeguarded Anderson acceleration of the iteration ("Acceleration"): 0 (default) = off,
 *                   1 .. 16 = keep the last m differences of the fixed-point map (X, sigma S) -> (X+, sigma S+) and extrapolate behind every
 *                   iteration; anything else is CUADMM_ERR_INVALID.  Costs (2 m + 3) 2 L doubles of device memory (two rings of m columns,
 *                   u_k, g_k, the fallback copy).  Runs one iteration per launch (no batches, no early y-solve); refused at init together
 *                   with world > 1, an in-process group or eig_rank > 0.  Set before cuadmm_init.
 *   "accel_safeguard"   default 2.0: the candidate behind iteration k is rejected (the iterate goes back to the plain f_k, the memory is
 *                   cleared, the iteration spent on it stays counted) when ||g_{k+1}|| > accel_safeguard ||g_k||; <= 0 rejects every candidate
 *   "accel_reg"     default 1e-10: the least-squares system is (G + accel_reg tr(G) / cols I) gamma = rhs
 *   "infeas_check"  period p of the infeasibility check ("Infeasibility certificates"): 0 (default) = off, an integer from 2 to
 *                   1 000 000 = every p iterations the differences y_k - y_{k-p}, X_k - X_{k-p} are tested for a certificate of primal or
 *                   dual infeasibility; a certificate ends the solve (cuadmm_get_status, cuadmm_get_certificate).  Anything else is
 *                   CUADMM_ERR_INVALID.  Costs 3 L + 3 m doubles of device memory and, from the first check that needs a projection,
 *                   a projection plan of its own.  Runs one iteration per launch (no batches, no early y-solve); refused at init together
 *                   with world > 1, an in-process group, eig_rank > 0 or accel > 0.  Weak infeasibility is not detected.  Set before cuadmm_init.
 *   "infeas_tol"    default 1e-6: a ray is a certificate when its violation eta is at most infeas_tol times its scalar (b'dy or -C'dx, per unit norm)
 *   "gap_check"     period p of the certified-gap check ("Certified lower bound"): 0 (default) = off, an integer from 2 to
 *                   1 000 000 = every p iterations the lower bound of cuadmm_lower_bound is formed at the iteration's y; the solve keeps the
 *                   best one (cuadmm_get_gap_info) and ends with status 5 when g = |pobj - LB| / (1 + |pobj| + |LB|) <= gap_tol and
 *                   errRp <= gap_tol.  Anything else is CUADMM_ERR_INVALID.  Needs trace bounds (cuadmm_set_trace_bounds before
 *                   cuadmm_init).  Costs 2 L + m doubles, the per-block lists and, from the first check, a projection plan of its own.
 *                   Runs one iteration per launch (no batches, no early y-solve); refused at init together with world > 1, an in-process
 *                   group, eig_rank > 0, accel > 0 or infeas_check > 0.  Without a verdict the run is the run with the option off, bit for
 *                   bit.  Set before cuadmm_init.
 *   "gap_tol"       default 0 = the solve's stop_tol: the tolerance of the certified-gap verdict
 *   "tail_shard"    world > 1, coupled constraints: 1 (default) = each rank applies 1 / world of the rows of the dense GPU tail of the
 *                   replicated y-solve and the K partial results are all-reduced; 0 = every rank applies the whole tail
 *   "tail_pivot"    1 (default) = the dense LDL^T of the y-solve's GPU tail pivots on the diagonal (P S P^T = L D L^T, |L_ij| <= 1): its explicit inverse stays
 *                   accurate where the Schur complement is nearly singular; 0 = the unpivoted elimination order (rounds 2 - 5)
 *   "tail_refine"   1 = one more accuracy device of the dense GPU tail of the y-solve: one refinement step of each triangular solve against the factor itself
 *                   (u <- u + W (z - L u), x <- x + W^T (v - L^T x)) on top of the explicit inverse W = inv(L22), whose accuracy is u cond(L22) -- a
 *                   nearly singular Schur complement (large moment relaxations) otherwise leaves 1e-8 ... 1e-7 in the primal objective against an exact
 *                   LDL^T solve (the reference's contract, include/cuadmm/cholesky_cpu.h:146-155).  Costs 6x the tail's bytes per solve and two more
 *                   K x K matrices; default 0.  cuadmm_get_tail_info [4] reports the measured accuracy of the explicit inverse.
 *   "psd_lg_fuse"   1 (default) = a handful of blocks of 65 <= n <= 512 run their whole projection -- svec -> dense, norm, every step of the matrix-sign
 *                   iteration, final product, svec store -- in ONE launch; 0 = prologue and epilogue as launches of their own (bit-identical)
 *   (every other switch: INTEGRATION.md section 6, which lists every key with its default)
 */
int cuadmm_set_option(cuadmm_solver* s, const char* key, double value);
/* Read-only views of the option tables, host only (no device is touched).  cuadmm_option_count: the number of keys.  cuadmm_option_info: row i
 * in table order, the engine's keys first, then the psd_* keys; any output pointer may be null.  *env: the environment variable that gives the
 * default, or null.  *def: the built-in default.  *flags: bits 0-1 kind (0 int, 1 long long, 2 real); bits 2-3 when the value is read (0 before
 * cuadmm_init only: refused afterwards, 1 by cuadmm_init, 2 when a projection plan is built, 3 while solving); bits 4-5 in-process group (0 shared
 * by all ranks, 1 per rank, 2 the leader's test hook); bit 6 the variable is negated (VAR != 0 means 0); bit 7 the variable also takes the
 * spellings eig / lds; bit 8 a psd_* key.  cuadmm_get_option: the value the solver holds for key, as a double. */
int cuadmm_option_count(void);
int cuadmm_option_info(int i, const char** key, const char** env, double* default_value, unsigned* flags);
int cuadmm_get_option(cuadmm_solver* s, const char* key, double* value);

/* Collective hook for block-sharded multi-GPU runs.  `fn` must sum
 * `count` doubles at device pointer `buf` over all ranks, in place, ordered on `hip_stream`
 * (a hipStream_t).  bench.py installs torch.distributed (RCCL) here; cuadmm_use_rccl
 * installs a direct RCCL communicator instead. */
typedef int (*cuadmm_allreduce_fn)(void* user, double* buf, size_t count, void* hip_stream);
int cuadmm_set_allreduce(cuadmm_solver* s, cuadmm_allreduce_fn fn, void* user);
/* Direct RCCL: `unique_id` is the 128-byte ncclUniqueId shared by all ranks
 * (cuadmm_rccl_unique_id fills one on rank 0). */
int cuadmm_rccl_unique_id(char out128[128]);
int cuadmm_use_rccl(cuadmm_solver* s, const char unique_id128[128], int rank, int world);

/* Block types: blk_vals[k] > 0 is a PSD block of that size ('s n' in blk.txt); blk_vals[k] < 0 is an UNCONSTRAINED block of
 * -blk_vals[k] variables ('u n', reference README.md:55-64, "WIP" there: its loader rejects it, problem.cu:28-36), which owns
 * that many svec slots and is left untouched by the cone projection.  cuadmm_problem_from_txt maps 'u n' lines to -n. */
/* SDPSolver::init  (reference include/cuadmm/solver.h:208-223, src/solver.cu:27-342).
 * Same argument list and meaning.  At is the CSC of A^T (vec_len x con_num): column j =
 * constraint j, row ids = svec indices.  X/y/S may be NULL (cold start, zeros).  Caller keeps
 * ownership of every array; they are copied.  `eig_stream_num_per_gpu` and
 * `cpu_eig_thread_num` are accepted for signature compatibility (the reference ignores the
 * latter too, solver.cu:29). */
int cuadmm_init(cuadmm_solver* s,
                int eig_stream_num_per_gpu, int cpu_eig_thread_num,
                int vec_len, int con_num,
                const int* At_csc_col_ptrs, const int* At_csc_row_ids, const double* At_csc_vals, int At_nnz,
                const int* b_indices, const double* b_vals, int b_nnz,
                const int* C_indices, const double* C_vals, int C_nnz,
                const int* blk_vals, int mat_num,
                const double* X, const double* y, const double* S,
                double sig);

/* SDPSolver::solve  (reference solver.h:236-244, src/solver.cu:355-823).  Reference
 * defaults: sig_update_threshold=500, stage_1=50, stage_2=100, switch_admm=11000,
 * sigscale=1.05, if_first=1. */
int cuadmm_solve(cuadmm_solver* s, int max_iter, double stop_tol,
                 int sig_update_threshold, int sig_update_stage_1, int sig_update_stage_2,
                 int switch_admm, double sigscale, int if_first);

/* SDPDuoSolver::init / ::solve  (reference include/cuadmm/duo_solver.h:236-276, src/duo_solver.cu): the
 * two-block-size specialisation (moment + localizing matrices).  Same iteration; the reference differs only in
 * where the moment-matrix eigendecompositions run (`if_gpu_eig_mom`: N GPUs through threads + P2P copies, or
 * `cpu_eig_thread_num` host LAPACK threads).  Here every block is projected by the kernels of this engine:
 *   if_gpu_eig_mom = 0 (host-LAPACK moment matrices) is REFUSED with CUADMM_ERR_INVALID unless option
 *     "duo_cpu_eig_on_gpu" = 1 says that running them on the GPU instead is what the caller wants;
 *   device_num_requested = N > 1 from ONE process runs N engines on N host threads (devices 0 .. N-1, or all on
 *     this solver's device with option "duo_share_device" = 1), blocks sharded by index, the exchange step an
 *     in-process all-reduce through peer-visible staging buffers; with rank / world already
 *     set by the caller (one process per GPU) N must equal world.
 * Like the reference (analyze_blk.cu:39-43) init rejects inputs that do not have exactly two distinct block sizes. */
int cuadmm_duo_init(cuadmm_solver* s,
                    int if_gpu_eig_mom, int device_num_requested,
                    int eig_stream_num_per_gpu, int cpu_eig_thread_num,
                    int vec_len, int con_num,
                    const int* At_csc_col_ptrs, const int* At_csc_row_ids, const double* At_csc_vals, int At_nnz,
                    const int* b_indices, const double* b_vals, int b_nnz,
                    const int* C_indices, const double* C_vals, int C_nnz,
                    const int* blk_vals, int mat_num,
                    const double* X, const double* y, const double* S,
                    double sig /* reference default 2e2 */);
int cuadmm_duo_solve(cuadmm_solver* s, int max_iter, double stop_tol,
                     int sig_update_threshold, int sig_update_stage_1, int sig_update_stage_2,
                     int switch_admm, double sigscale, int if_first);

/* Results: the reference exposes public members X.vals / y.vals / S.vals (device pointers,
 * unscaled after solve, solver.cu:814-816) and info_* vectors (solver.h:149-161). */
int cuadmm_get_dims(const cuadmm_solver* s, int* vec_len, int* con_num, int* mat_num);
int cuadmm_get_X(cuadmm_solver* s, double* host_out /* vec_len */);
int cuadmm_get_y(cuadmm_solver* s, double* host_out /* con_num */);
int cuadmm_get_S(cuadmm_solver* s, double* host_out /* vec_len */);
/* replace the (unscaled) iterate between two solve() calls, as the reference allows by
 * writing through X.vals/y.vals/S.vals before solve(..., if_first=false) (solver.cu:385-409);
 * NULL leaves that vector untouched */
int cuadmm_set_XyS(cuadmm_solver* s, const double* X, const double* y, const double* S, double sig);
/* W_k = M_k V_k for every PSD block k of the resident point: M = X (which = 0), S (1) or S^ = C - A'y at the current y (2); V_k is n_k x r_k,
 * r_k = ranks[k] ("Blocks times factors"; csrc/block_mult.h).  V and W_out hold cuadmm_lowrank_size(rmax) doubles in the layout
 * of cuadmm_lowrank's L_out for this rmax: block k at the prefix sum of n_j min(n_j, rmax) over the PSD blocks before it, column by
 * column, n_k doubles per column; unconstrained blocks occupy nothing, are not read, and their entries of ranks (mat_num ints) are
 * ignored.  Columns >= r_k of V are never read (they may hold NaN); in W_out they are +0.0 (r_k = 0: the whole block).
 * One kernel pass on the fp64 matrix cores reads the svec slots where they lie and forms, with s_ij the raw slot of (i, j),
 *   W[i, t] = sign * fma(0.7071067811865476, sum_{j != i} s_ij V[j, t], s_ii * V[i, t])        (sign = -1 for which = 2, else 1),
 * every row of W owned by one wavefront (no atomics: the same bits on every run).  For any order of the sums, with u = 2^-53 and M_ij
 * the exact matrix entry (s_ij / sqrt(2) or s_ii),
 *   |W[i, t] - exact| <= (n_k + 4) u sum_j |M_ij| |V[j, t]|
 * (n_k products and sums, the scaling, the constant's own rounding and one spare); with small-integer slots and V the result is the
 * correctly rounded value of the exact one.  For which = 2 the vector is formed as cuadmm_lambda_min forms it, -(A'y - C) by the
 * iteration's kernel in the engine's scaled space, and its own rounding comes on top.  Behind a solve the scaled iterate is read and W
 * is multiplied on the host by the unit (bscale for X, Cscale for S and S^: one more u); the deferred unscaling is not triggered and a
 * following cuadmm_solve(..., if_first = 0) continues bit for bit.  Nothing of the solver changes.
 * per_block (may be NULL), 4 mat_num doubles: [4k] ||W_k||_F, [4k + 1] <V_k, W_k>, [4k + 2] ||V_k||_F, [4k + 3] flag: 0 multiplied, 2
 * unconstrained (then the three numbers are 0).  They are formed on the host from the returned W_out and V over the entries e of the
 * r_k columns in index order with plain doubles: q = 0; q = q + a[e] * b[e] (the product rounded, then the sum), the norms the square
 * roots of such sums.
 * out8: [0] sqrt of the sum over k, in block order, of the sums of squares behind [4k]; [1] the sum over k of [4k + 1]; [2] the PSD
 * block with the largest ||W_k||_F, the first of equals (-1: no PSD block); [3] that norm; [4] PSD blocks; [5] sum of r_k; [6] device
 * milliseconds of the kernel pass (HIP events), with the formation of S^ for which = 2 -- the staged copy of V to the device and of W
 * back, both whole buffers, are not in it; [7] bytes of device memory the call holds.
 * CUADMM_ERR_INVALID, the solver as it was: solver not initialised; out8, W_out or ranks NULL; which outside 0..2; rmax outside 1..8192;
 * a ranks[k] of a PSD block outside 0..min(n_k, rmax); V NULL while some rank is positive; an entry that is not finite in a column
 * that would be read; world > 1 or a handle that leads an in-process group.  CUADMM_ERR_FACTOR for which = 2 behind a failed
 * cuadmm_update_A. */
int cuadmm_block_multiply(cuadmm_solver* s, int which, const double* V, const int* ranks, int rmax, double* W_out, double out8[8], double* per_block);
/* Value and gradient of the augmented Lagrangian at per-block factors ("Value and gradient at factors"; csrc/lowrank_grad.h).
 * With x the resident X in which every PSD block k is replaced by L_k L_k' (unconstrained blocks keep their resident slices), y the
 * caller's vector of con_num doubles (NULL: the resident y) and sigma >= 0 in the caller's units (not the solver's sig):
 *   r = A x - b,   f = <C, x> - y'r + (sigma / 2) ||r||^2,   ytilde = y - sigma r,   S^ = C - A'ytilde,   G_k = 2 S^_k L_k.
 * G is the gradient of f with respect to the factors, the unconstrained slices of S^ the gradient with respect to those slices of x.
 * L, ranks, rmax and G_out as V, ranks, rmax and W_out of cuadmm_block_multiply: columns >= r_k of L are never read (they may hold NaN)
 * and are +0.0 in G_out.  G_out (cuadmm_lowrank_size(rmax) doubles), r_out (con_num, the caller's order), Shat_out (vec_len; one more
 * copy back when asked for) and per_block may be NULL.
 * The chain runs on the solver's stream in the engine's scaled space: a device copy of X into a vector of the call's own, svec(L_k L_k')
 * over its PSD blocks (the kernel of cuadmm_set_lowrank), A x (the iteration's SpMV), one streaming pass that forms r, ytilde and the
 * slot sums of y'r and ||r||^2, A'ytilde - C (the iteration's kernel), the product of cuadmm_block_multiply(2) and one pass of per-block
 * sums.  No atomics: the same bits on every run.  With sigma = 0, ytilde is y bit for bit and G is bit for bit 2 W of
 * cuadmm_block_multiply(s, 2, L, ...) at the same y.  Nothing the iteration reads is written and the deferred unscaling is not
 * triggered: a following cuadmm_solve(..., if_first = 0) continues bit for bit.
 * out8: [0] f, [1] <C, x> (the sum over k of [4k] in block order), [2] y'r, [3] ||r||, [4] ||G||_F, [5] <L, G> (= 2 <S^, x> on the PSD
 * part), [6] device milliseconds of the chain (HIP events; the staged copies are not in it), [7] bytes of device memory the call holds.
 * per_block, 4 mat_num doubles: [4k] <C_k, x_k>, [4k + 1] ||G_k||_F (unconstrained: ||S^_k||_F), [4k + 2] <L_k, G_k> (unconstrained: 0),
 * [4k + 3] ||L_k||_F^2 (unconstrained: 0).  The sums over G and L are formed on the host from the returned G_out and L as
 * cuadmm_block_multiply forms its own: q = 0; q = q + a[e] * b[e] in index order, [4] from the blocks' sums of squares in block order.
 * CUADMM_ERR_INVALID, the solver as it was: solver not initialised; out8 or ranks NULL; sigma negative or not finite; rmax outside
 * 1..8192; a ranks[k] of a PSD block outside 0..min(n_k, rmax); L NULL while some rank is positive; an entry of y or of a column of L that
 * would be read that is not finite; world > 1 or a handle that leads an in-process group.  CUADMM_ERR_FACTOR behind a failed
 * cuadmm_update_A. */
int cuadmm_lowrank_grad(cuadmm_solver* s, const double* L, const int* ranks, int rmax, const double* y, double sigma, double* G_out, double* r_out,
                        double* Shat_out, double out8[8], double* per_block);
/* The augmented Lagrangian of cuadmm_lowrank_grad along a line in factor space, as an exact quartic ("Line search along factor
 * steps"; csrc/lowrank_line.h).  With x(t) the resident X in which every PSD block k is replaced by (L_k + t D_k)(L_k + t D_k)'
 * (unconstrained blocks keep their resident slices for every t), y and sigma as in cuadmm_lowrank_grad:
 *   x(t) = x0 + t x1 + t^2 x2,  x0 = L L',  x1 = L D' + D L',  x2 = D D';    r(t) = r0 + t p + t^2 q,  r0 = A x0 - b,  p = A x1,  q = A x2
 *   f(t) = <C, x(t)> - y'r(t) + (sigma / 2) ||r(t)||^2 = c0 + c1 t + c2 t^2 + c3 t^3 + c4 t^4
 *   c0 = <C, x0> - y'r0 + (sigma / 2) r0'r0      c1 = <C, x1> - y'p + sigma r0'p      c2 = <C, x2> - y'q + (sigma / 2)(p'p + 2 r0'q)
 *   c3 = sigma p'q                               c4 = (sigma / 2) q'q
 * L, ranks, rmax as in cuadmm_lowrank_grad; D has the layout and the ranks of L.  Columns >= r_k of L and of D are never read (they may
 * hold NaN).  coef5 <- c0 .. c4.  r_out, p_out, q_out (con_num doubles each, the caller's order) and per_block may be NULL.
 * The chain runs on the solver's stream in the engine's scaled space: a device copy of X into the call's own x0, one launch that forms
 * svec of the three outer products over the PSD blocks of x0, x1, x2 (three accumulators per 16 x 16 tile on the fp64 matrix cores; x0 is
 * bit for bit the vector cuadmm_lowrank_grad assembles), the iteration's SpMV three times, one streaming pass that forms r0, p, q and
 * nine slot sums, one pass of per-block sums.  No atomics: the same bits on every run.  r_out is bit for bit cuadmm_lowrank_grad's r_out
 * at the same L, y, sigma.  Negating D negates c1 and c3 bit for bit and keeps c0, c2, c4.  Nothing the iteration reads is written and the
 * deferred unscaling is not triggered: a following cuadmm_solve(..., if_first = 0) continues bit for bit.
 * t_max > 0 (+inf included): the coefficients go through cuadmm_quartic_min(coef5, t_max, .).  t_max <= 0: coefficients only.
 * out8: [0] t* (t_max <= 0: 0), [1] f(t*) by Horner (t_max <= 0: c0), [2] f(t*) - c0, [3] ||p||, [4] ||q||, [5] interior critical points
 * found, [6] device milliseconds of the chain (HIP events; the staged copies are not in it), [7] bytes of device memory the call holds.
 * per_block, 4 mat_num doubles: [4k] <C_k, x0_k>, [4k + 1] <C_k, x1_k>, [4k + 2] <C_k, x2_k>, [4k + 3] 0 for a PSD block, 2 for an
 * unconstrained one (there [4k + 1] = [4k + 2] = 0).
 * Rounding (u = 2^-53, gamma(K) = K u / (1 - K u) times the absolute-value chain of each quantity; c / c' the most entries in a row of
 * A / A', R the largest rank), counted launch by launch as for cuadmm_lowrank_grad.  A slot of x0 or x2: the outer product's R + 4 and 6
 * for the factors' unit (or 2 for fl(1 / bscale) in A x), R + 10; a slot of x1: 2 R + 10.
 *   r0, q  K_r = c + R + 16 (cuadmm_lowrank_grad's; q has no b and lies inside it)        p  K_p = c + 2 R + 16
 *   <C, x0>, <C, x2>  K_cx = vec_len + R + 16                                               <C, x1>  K_cx1 = vec_len + 2 R + 16
 *   y'v   K_v + m + 270 for v = r0, p, q                 v'w   K_v + K_w + m + 266 for v, w among r0, p, q
 *   c0  max(K_cx, K_r + m + 270, 2 K_r + m + 266) + 2 (= cuadmm_lowrank_grad's K_f)         c1  max(K_cx1, K_p + m + 270, K_r + K_p + m + 266) + 3
 *   c2  max(K_cx, K_r + m + 270, 2 K_p + m + 266) + 4        c3  K_p + K_r + m + 268        c4  2 K_r + m + 268
 * (tests/_lowrank_line_twin.py has the chains.)
 * CUADMM_ERR_INVALID, the solver and every output as they were: the list of cuadmm_lowrank_grad, applied to L and to D (D NULL while some
 * rank is positive; an entry of a column of D that would be read that is not finite); coef5 NULL; t_max NaN; a t_max > 0 that
 * cuadmm_quartic_min refuses for these coefficients (+inf on a quartic that is not bounded below).  CUADMM_ERR_FACTOR behind a failed
 * cuadmm_update_A. */
int cuadmm_lowrank_line(cuadmm_solver* s, const double* L, const double* D, const int* ranks, int rmax, const double* y, double sigma, double t_max,
                        double coef5[5], double* r_out, double* p_out, double* q_out, double out8[8], double* per_block);
/* The global minimiser of c[0] + c[1] t + c[2] t^2 + c[3] t^3 + c[4] t^4 on [0, t_max].  Host only: no device, no solver handle.
 * t_max = +inf is allowed where c[4] > 0, or c[4] = c[3] = 0 and c[2] > 0.  Candidates: 0, a finite t_max and the real roots of the
 * derivative inside the interval (bracketed by the closed-form stationary points of the derivative, refined by Newton steps safeguarded
 * by bisection); each is evaluated by Horner, the smallest value wins, ties go to the smallest t.
 * out4: [0] t*, [1] f(t*), [2] f(t*) - c[0], [3] interior critical points found.
 * CUADMM_ERR_INVALID: c or out4 NULL, a coefficient that is not finite, t_max negative or NaN, t_max = +inf on a quartic that is not
 * bounded below by the rule above. */
int cuadmm_quartic_min(const double c[5], double t_max, double out4[4]);
/* `steps` iterations of Polak-Ribiere+ nonlinear conjugate gradients on cuadmm_lowrank_grad's f over the factors of the PSD blocks, with
 * the exact line search of cuadmm_lowrank_line, and the factors, the direction and the gradients resident on the device throughout
 * ("Refinement over factors"; csrc/lowrank_refine.h).  L, ranks, rmax, y, sigma as in cuadmm_lowrank_grad: columns >= r_k of L
 * are never read (they may hold NaN).  y and sigma are fixed for the whole call.  All scalars are fp64, every operation rounded once.
 * Step k = 0, 1, ... with e over the cuadmm_lowrank_size(rmax) entries:
 *   1. G = the gradient at L_k, bit for bit cuadmm_lowrank_grad's G_out (that chain without its per-block terms);
 *   2. gg = sum G^2, go = sum G G_old, gd = sum G D_old (one kernel; 256 slot partials each, added in slot order; G_old = D_old = 0 at k = 0);
 *   3. [beta, slope, restart] = cuadmm_cg_update(gg, go, gd, gg of the step before, k == 0);  D[e] = fl(fl(beta D_old[e]) - G[e]), on a
 *      restart - G[e];  G_old = G;
 *   4. c0 .. c4 bit for bit cuadmm_lowrank_line(L_k, D_k)'s coef5 (that chain) and [t, f(t)] = cuadmm_quartic_min(c, t_max, .);
 *   5. L_{k+1}[e] = fl(L_k[e] + fl(t D_k[e])).
 * Behind a solve, where X lies scaled, the copies of L and D in X's units are fl(. root), root = fl(1 / sqrt(bscale)), formed on the
 * device as cuadmm_lowrank_grad and cuadmm_lowrank_line form them on the host.  No atomics: the same bits on every run.  The host waits
 * for the device twice per step (the three sums; the quartic's partials); nothing else crosses.
 * The loop ends with reason 0: `steps` steps done; 1: t == 0, the step is not taken; 2: gtol > 0 and sqrt(gg) <= gtol, tested before the
 * line search (gtol in the caller's units, 0: never); 3: a sum or a coefficient is not finite; 4: cuadmm_quartic_min refuses (t_max =
 * +inf on a quartic that is not bounded below: sigma = 0, or A (D D') = 0).  Every reason returns CUADMM_OK with the factors behind the
 * last step taken.
 * L_out: cuadmm_lowrank_size(rmax) doubles, + 0.0 in the columns >= r_k; it may alias L.
 * trace: 16 doubles per step, room for `steps` rows; row k = [gg, go, gd, beta, slope, restart, c0, c1, c2, c3, c4, t, f(t), device
 * milliseconds of the step (HIP events), 0, 0].  f at L_k is c0.  A step that ends the loop early leaves a last row with what it had
 * formed and 0 elsewhere; the rows behind it are not written.
 * out8: [0] steps taken, [1] reason, [2] c0 of the first step (NaN where none was formed), [3] the last f(t) (NaN where none),
 * [4] the last sqrt(gg), [5] device milliseconds of the whole loop, [6] bytes of device memory the call holds, [7] 0.
 * r_out (con_num doubles, the caller's order; may be NULL): r = A x - b at the factors of the last step begun (cuadmm_lowrank_line's r_out
 * there, bit for bit); r(t) = r + t p + t^2 q is not formed.
 * Nothing the iteration reads is written and the deferred unscaling is not triggered: a following cuadmm_solve(..., if_first = 0)
 * continues bit for bit.  X is not changed: the caller passes L_out to cuadmm_set_lowrank.  Not in the call: updates of y or an outer
 * augmented-Lagrangian loop, rank adaptation, preconditioning.
 * CUADMM_ERR_INVALID, the solver and every output as they were: the list of cuadmm_lowrank_grad; L_out, trace or out8 NULL; steps < 1;
 * t_max <= 0 or NaN; gtol negative or not finite.  CUADMM_ERR_FACTOR behind a failed cuadmm_update_A. */
int cuadmm_lowrank_refine(cuadmm_solver* s, const double* L, const int* ranks, int rmax, const double* y, double sigma, int steps, double t_max, double gtol,
                          double* L_out, double* trace, double out8[8], double* r_out);
/* The scalar step of cuadmm_lowrank_refine between a gradient and a direction.  Host only: no device, no solver handle.  Plain doubles:
 *   beta = max(0, (gg - go) / gg_prev), 0 where first != 0 or gg_prev == 0;   slope = beta gd - gg;   restart = first != 0 or not slope < 0.
 * out3: [0] beta (0 on a restart), [1] slope as formed above, [2] restart (1 or 0).
 * CUADMM_ERR_INVALID: out3 NULL, or one of gg, go, gd, gg_prev not finite. */
int cuadmm_cg_update(double gg, double go, double gd, double gg_prev, int first, double out3[3]);
/* Replace X (which = 0) or S (1) between two solves by per-block factors: every PSD block k becomes L_k L_k' with r_k = ranks[k] columns
 * ("Starting from low-rank factors"; csrc/lowrank_apply.h).  L is laid out as cuadmm_lowrank's L_out for this rmax: block k at the
 * prefix sum of n_j min(n_j, rmax) over the PSD blocks before it, column by column, n_k doubles per column; unconstrained blocks occupy
 * nothing and their entries of ranks (mat_num ints) are ignored.  Columns >= r_k are never read (they may hold NaN); r_k = 0 writes +0.0.
 * One kernel pass on the fp64 matrix cores writes v[off_k + i (i + 1) / 2 + j] = c_ij sum_t L[i, t] L[j, t] (i >= j, c_ii = 1, c_ij =
 * 1.4142135623730951) into the resident vector; for any order of the sums, with u = 2^-53,
 *   |computed - exact| <= (r_k + 4) u c_ij sum_t |L_it| |L_jt|
 * (r_k products and sums, the multiplication by the constant, the constant's own rounding).
 * Otherwise the call is cuadmm_set_XyS for that one vector, in the caller's units: the deferred unscaling runs first, sig > 0 sets sigma,
 * status, infeasibility snapshots and gap information are reset; y, the other matrix and the unconstrained blocks of the target keep
 * their bits (set those through cuadmm_set_XyS first where needed).
 * out4 (may be NULL): [0] PSD blocks written, [1] sum of r_k, [2] device milliseconds of the kernel pass (HIP events), [3] bytes of
 * factors staged from the host: 8 sum n_k min(n_k, rmax) -- the factor buffer travels whole, in one copy -- or 0 where L is NULL (the
 * 4 mat_num bytes of ranks are not counted).
 * Refused with CUADMM_ERR_INVALID before anything changes (the deferred unscaling included), the solver left as it was: solver not
 * initialised; which outside 0..1; rmax outside 1..8192; ranks NULL; a ranks[k] of a PSD block outside 0..min(n_k, rmax); L NULL while
 * some rank is positive; an entry that is not finite in a column that would be read; world > 1 or a handle that leads an in-process
 * group (one rank only, like cuadmm_lowrank). */
int cuadmm_set_lowrank(cuadmm_solver* s, int which, const double* L, const int* ranks, int rmax, double sig, double out4[4]);
/* Replace b and/or C of an initialised solver without touching anything that depends on A alone (ordering, factor, GPU tail,
 * tree tops, plans).  b / C in the caller's numbering and units exactly as in cuadmm_init; b_nnz < 0 (or C_nnz < 0) leaves that
 * one unchanged.  keep_iterate = 1: the current X, y, S (caller's units) become the start of the next solve (warm start);
 * 0: zeros, as cuadmm_init with NULL X / y / S.  sig > 0 sets sigma, otherwise the current value stays.
 * Afterwards the solver is in the state cuadmm_init(At, blk, same options, new b, new C, X0, y0, S0, sig) would have left:
 * scaling constants, info arrays, total_time, best iterate and schedule hints as after init; profile counters and plans stay.
 * Every index is checked before anything changes (range; no index twice, anywhere in b or C): a refused call returns
 * CUADMM_ERR_INVALID and leaves the solver as it was.  Every rank of a sharded job calls it with the full b and C; the leader
 * of an in-process group forwards it to its engines.  Not in the reference, whose only way to new data is a second init. */
int cuadmm_update_bC(cuadmm_solver* s, const int* b_indices, const double* b_vals, int b_nnz,
                     const int* C_indices, const double* C_vals, int C_nnz, int keep_iterate, double sig);
/* New values of A on the pattern given to cuadmm_init.  At_csc_vals has At_nnz entries in the caller's order at init (same
 * col_ptrs / row_ids, not passed again).  b, C, options, block structure stay.  keep_iterate / sig as in cuadmm_update_bC.
 * Afterwards the solver is in the state cuadmm_init(same pattern, blk, b, C, options; the new values; the current iterate in the
 * caller's units or zeros) would have left, bit for bit: scaling constants, column norms, info arrays, total_time, best iterate, schedule
 * hints and acceleration memory as after init; profile counters and plans stay.  The ordering and the symbolic analysis of A A^T do
 * not run: the host factor is refactored on the analysis of init (cuadmm_aat_refactor), the GPU tail, the streams of the device-side
 * y-solve, the value arrays of A and A^T, the closed blocks' records and b are formed again by the routines of init.
 * Checked before anything changes (CUADMM_ERR_INVALID, solver as it was): At_nnz equals the count at init; every value is finite.
 * EXPLICIT ZEROS: cuadmm_init keeps every entry it is given in the pattern, also one whose value is exactly 0 (nothing is dropped from A,
 * from A A^T or from the factor), so a value of exactly 0 is accepted here like any other.
 * If the new A A^T cannot be factored -- a zero or non-finite pivot, a GPU tail that fails its factorisation or probe solve, or a
 * value-dependent decision of init that would come out differently -- the call returns CUADMM_ERR_FACTOR and
 * cuadmm_solve / cuadmm_update_bC refuse with that code until a later cuadmm_update_A succeeds.  After CUADMM_ERR_FACTOR the handle
 * holds a mixture of old and new data: only reading X, y, S (the caller's units, unchanged) and a further cuadmm_update_A are defined.
 * Every rank of a sharded job calls it with the full value array, as with init; the leader of an in-process group forwards it to its
 * engines.  With owned constraints a rank whose factorisation fails fails the call on every rank; a rank that returns earlier than
 * that -- a HIP error while it brings X, y, S back to the caller's units -- does so alone, and the job must be ended as after any
 * rank's HIP error.  Not in the reference. */
int cuadmm_update_A(cuadmm_solver* s, const double* At_csc_vals, int At_nnz, int keep_iterate, double sig);
/* [0] updates so far, [1] wall ms of the last one, [2] host numeric factor ms, [3] device part of the y-solve rebuild ms,
 * [4] orderings run on this handle since create (stays 1; 2 on a handle whose init fell back from the GPU tail to the host-only factor,
 * which refuses cuadmm_update_A), [5] bytes that crossed to the device in the last update */
int cuadmm_get_update_info(const cuadmm_solver* s, double out6[6]);
/* option profile = 1: the two streaming passes of the last cuadmm_update_A, each timed alone by events: [0] ms and [1] bytes (index
 * maps read, values gathered and stored) of the value pass's kernel, [2] ms and [3] bytes of the svec pass over X and S */
int cuadmm_get_update_pass_info(const cuadmm_solver* s, double out4[4]);
/* device pointers of this rank's shard (scaled inside solve, unscaled after) */
int cuadmm_get_device_ptrs(cuadmm_solver* s, double** X, double** y, double** S);
/* svec range [begin,end) owned by this rank (whole vector when world==1) */
int cuadmm_get_shard(const cuadmm_solver* s, int64_t* svec_begin, int64_t* svec_end, int* blk_begin, int* blk_end);

#define CUADMM_INFO_POBJ 0
#define CUADMM_INFO_DOBJ 1
#define CUADMM_INFO_ERRRP 2
#define CUADMM_INFO_ERRRD 3
#define CUADMM_INFO_RELGAP 4
#define CUADMM_INFO_SIG 5
#define CUADMM_INFO_BSCALE 6
#define CUADMM_INFO_CSCALE 7
int cuadmm_get_info_iter_num(const cuadmm_solver* s);
/* copies min(cap, iter_num) entries of info_<which>_arr; returns the number copied */
int cuadmm_get_info_array(const cuadmm_solver* s, int which, double* out, int cap);
double cuadmm_get_total_time(const cuadmm_solver* s);
/* scalars of the current state: errRp, errRd, pobj, dobj, relgap, sig, bscale, Cscale,
 * norm_borg, norm_Corg, best_KKT, eig_not_converged (12 doubles) */
int cuadmm_get_state(const cuadmm_solver* s, double out12[12]);

/* Per-kernel-class timing collected when option "profile"=1 (HIP events on the engine
 * stream).  Classes: 0 aty_xb, 1 psd_project, 2 post_proj, 3 spmv_A, 4 copies/h2d/d2h,
 * 5 host_solve (wall, without 7), 6 allreduce, 7 GPU part of the A*A^T solve (wall, incl. transfers).  out[3*k+0]=launches, [3*k+1]=total ms, [3*k+2]=bytes
 * (algorithmic HBM bytes per launch).  */
#define CUADMM_NUM_KCLASS 8
int cuadmm_get_profile(const cuadmm_solver* s, double out[3 * CUADMM_NUM_KCLASS]);
int cuadmm_reset_profile(cuadmm_solver* s);
/* Steps of the last projection per block of this rank's shard (0 for blocks served by the eigensolver kernels); needs
 * option "psd_steps".  Returns the number of entries written (<= cap) or a negative error code. */
int cuadmm_get_psd_steps(cuadmm_solver* s, int* out, int cap);
/* Counters of the engine's execution plan (diagnostics; what bench.py reports beside its numbers):
 *   [0] launches that ran several ADMM iterations (option "batch"), [1] iterations run by them, [2] batches rolled back because
 *   the stopping test fired inside them, [3] threads of the host pool, [4] 1 if the iteration is fused into the projection
 *   kernels, [5] 1 if every block solves for its own multipliers (closed blocks), [6] 1 if the y-solve runs on the device (2: hybrid --
 *   L11 sweeps on the host, L21 products and the tail on the device; 3: on the device with dense tree tops, option "lead_tops"),
 *   [7] size of the GPU tail of the A A^T factor. */
int cuadmm_get_counters(const cuadmm_solver* s, double out8[8]);
/* The dense GPU tail of the A A^T factor on this rank: [0] its size k (0: none), [1] bytes of inv(L22) this rank read in its last
 * solve (4 K^2 for the whole triangle; 1 / world of it when the tail is sharded, option "tail_shard"), [2] the rows it applied,
 * [3] bytes of device memory the tail holds on this rank, [4] accuracy of its explicit inverse W = inv(L22) measured at init,
 * || z - L22 (W z) ||_inf for a probe vector z of entries in [0.5, 1.5] (~ unit roundoff x cond(L22); -1: not measured), [5] 1 when option
 * "tail_refine" is on: every triangular solve of the tail takes one refinement step against the factor itself (6x the bytes per solve). */
int cuadmm_get_tail_info(const cuadmm_solver* s, double out[6]);
/* Option "accel": [0] memory m, [1] candidates taken, [2] accepted, [3] rejected, [4] restarts (the memory cleared because the map
 * changed: sigma, tau, the switch to ADMM, a degenerate least-squares system), [5] columns held now, [6] total ms in the acceleration
 * kernels when option "profile" is on (else 0; they are not part of cuadmm_get_profile), [7] bytes the two rings hold. */
int cuadmm_get_accel_info(const cuadmm_solver* s, double out8[8]);
/* The least-squares solve of the acceleration: (gram + reg tr(gram) / cols I) gamma = rhs, gram cols x cols row-major and symmetric,
 * 1 <= cols <= 16, by Cholesky in long double.  Host only (no device needed).  CUADMM_ERR_FACTOR when a pivot is not positive. */
int cuadmm_accel_solve_ls(const double* gram, const double* rhs, int cols, double reg, double* gamma_out);
/* How the last cuadmm_solve ended.  [0] status: 0 = no solve yet (or the problem / iterate was replaced since: cuadmm_update_bC,
 * cuadmm_update_A, cuadmm_set_XyS, cuadmm_set_lowrank), 1 = converged, 2 = iteration limit, 3 = primal infeasible, 4 = dual infeasible (primal unbounded),
 * 5 = certified gap (option "gap_check": cuadmm_get_gap_info has the bound);
 * [1] iteration of the verdict; then, of option "infeas_check" (zeros while it is off): [2] checks run in that solve, [3] beta = b'dy / ||dy||
 * (status 3) or gamma = -C'dX / ||dX|| (status 4) in the engine's scaled space, [4] eta = ||P+(A'dy)|| / ||dy|| (status 3) or
 * max(||A dX||, ||P+(-dX)||) / ||dX|| (status 4), [5] the certified radius in the caller's units: status 3: no X >= 0 with A X = b has
 * ||X||_F < [5]; status 4: no (y, S >= 0) with A'y + S = C has ||D y|| + ||S||_F < [5], D = diag(max(1, ||row_i of A||)) (infinite when
 * eta = 0), [6] milliseconds of device time spent in the checks of that solve (HIP events), [7] bytes of device memory the check holds:
 * its vectors exactly, plus an estimate of the second projection plan (the drop of the device's free memory around its build).
 * Statuses 1 and 2 are reported with the option off too. */
int cuadmm_get_status(const cuadmm_solver* s, double out8[8]);
/* The ray behind status 3 or 4, in the caller's units and order.  Status 3: y_out (con_num doubles) with b'y = 1 and A'y <= 0 up to
 * [4] / [3] of cuadmm_get_status; X_out may be null.  Status 4: X_out (vec_len doubles) with <C, X> = -1, A X = 0 and X >= 0 on the PSD
 * blocks up to the same ratio (its slices of unconstrained blocks are free); y_out may be null.  Any other status: CUADMM_ERR_INVALID. */
int cuadmm_get_certificate(cuadmm_solver* s, double* y_out, double* X_out);
/* The rule of the infeasibility check on the statistics of one check: stats = [||dy||^2, b'dy, ||dX||^2, C'dX, ||P+(A'dy)||^2, ||A dX||^2,
 * ||P+(-dX)||^2, unused].  verdict: 3 when b'dy > 0 and ||P+(A'dy)|| <= tol b'dy, else 4 when C'dX < 0 and max(||A dX||, ||P+(-dX)||) <=
 * -tol C'dX, else 0 (a NaN in a test's numbers: no verdict from it); radius (may be null): scalar / eta in the scaled space, infinite when
 * eta = 0.  Host only (no device needed). */
int cuadmm_infeas_decide(const double stats[8], double tol, int* verdict, double* radius);
/* Trace bounds for the certified lower bound ("Certified lower bound"): one number R_k >= 0 per block of blk_vals, in the
 * caller's units -- PSD block: every feasible X has tr X_k <= R_k; unconstrained block: ||x_k||_2 <= R_k.  They are a property of the
 * feasible set the caller asserts: the values are copied and survive cuadmm_update_bC / cuadmm_update_A.  R = NULL clears them (refused
 * on an initialised solver with option "gap_check" on).  A value that is negative or not finite, or a mat_num that is not the problem's
 * (checked here on an initialised solver, else at cuadmm_init): CUADMM_ERR_INVALID, and the solver keeps what it had.  Before or after
 * cuadmm_init. */
int cuadmm_set_trace_bounds(cuadmm_solver* s, const double* R, int mat_num);
/* A lower bound on the optimal value that holds for EVERY y: with S^ = C - A'y,
 *   LB(y) = b'y - sum_k R_k nubar_k,  nubar_k = ||P+(-S^_k)||_F + 2e-12 sqrt(2 len_k) ||S^_k||_F (PSD block), ||S^_k||_2 (unconstrained),
 * evaluated at the y cuadmm_get_y would return, on any initialised solver with trace bounds set (before a solve, after one, between
 * solve(..., if_first = 0) calls, after solves with any option); refused for world > 1 and in-process groups (CUADMM_ERR_INVALID) and,
 * as cuadmm_evaluate, behind a failed cuadmm_update_A (CUADMM_ERR_FACTOR: A', C, b and the scaling are half updated).  It changes nothing the
 * iteration reads: a following cuadmm_solve continues bit for bit as without the call.  The second term of nubar_k is the projection
 * kernels' accuracy; the rounding of A'y - C itself is not covered.  out8 (caller's units): [0] LB, [1] b'y, [2] sum R_k nubar_k,
 * [3] g = |pobj - LB| / (1 + |pobj| + |LB|) against the pobj of the current state, [4] the block with the largest term, [5] its term
 * R_k nubar_k, [6] milliseconds of device time (HIP events), [7] bytes of device memory the bound holds (its vectors exactly, plus an
 * estimate of its projection plan).  per_block (may be NULL): 2 mat_num doubles, [2k] nu_k = ||P+(-S^_k)||_F or ||S^_k||_2, [2k + 1] ||S^_k||_F. */
int cuadmm_lower_bound(cuadmm_solver* s, double out8[8], double* per_block);
/* Option "gap_check" in the last cuadmm_solve: [0] checks run, [1] the best (largest) lower bound of that solve -- every one of them is
 * valid --, [2] its iteration, [3] the last bound, [4] the last g, [5] milliseconds of device time in the checks, [6] bytes held (as [7]
 * of cuadmm_lower_bound), [7] iteration of the status-5 verdict or 0.  Zeros while the option is off; cleared where the status is. */
int cuadmm_get_gap_info(const cuadmm_solver* s, double out8[8]);
/* KKT and DIMACS report of any point (X, y, S) ("Evaluation of a point").  X, y, S: host pointers in the caller's units and
 * order, vec_len, con_num and vec_len doubles as cuadmm_set_XyS takes them; NULL: the vector cuadmm_get_X / _y / _S would return now
 * (behind a solve the scaled iterate is read where it lies: the deferred unscaling is not triggered).  With P+ the projection onto the
 * PSD cone of a block, Rd = A'y + S - C and ||.|| the 2-norm of the svec (the Frobenius norm of the block), all in the caller's units:
 *   per_block (may be NULL; 6 mat_num doubles), [6k + ...]: [0] ||X_k||, [1] vX_k = ||P+(-X_k)||, [2] ||S_k||, [3] vS_k = ||P+(-S_k)||,
 *     [4] <X_k, S_k>, [5] ||Rd_k||.  An unconstrained block has the whole space as its primal cone and {0} as its dual cone:
 *     vX_k = 0, vS_k = ||S_k||.
 *   out16: [0] pobj = <C, X>, [1] dobj = b'y, [2] ||A X - b||, [3] ||Rd||, [4] vX = sqrt(sum vX_k^2), [5] vS = sqrt(sum vS_k^2),
 *     [6] <X, S>, [7] ||b||, [8] ||C||, and the six DIMACS error measures [9] err1 = [2] / (1 + ||b||), [10] err2 = vX / (1 + ||b||),
 *     [11] err3 = [3] / (1 + ||C||), [12] err4 = vS / (1 + ||C||), [13] err5 = (pobj - dobj) / (1 + |pobj| + |dobj|),
 *     [14] err6 = <X, S> / (1 + |pobj| + |dobj|) (both signed), [15] milliseconds of device time (HIP events on the engine's stream).
 * Where DIMACS has max(0, -lambda_min(.)) in err2 and err4, this report has ||P+(-.)||_F, the 2-norm of ALL negative eigenvalues of all
 * blocks: the projection path has no eigenvalues.  That value lies between DIMACS's and sqrt(n) times it (n: the sum of the block
 * sizes) and is zero exactly when DIMACS's is.  The projections are the iteration's kernels, accurate to 2e-12 sqrt(2) ||M_k|| per
 * entry: vX_k, vS_k below that times sqrt(len_k) are rounding.
 * The call changes nothing the iteration reads: a following cuadmm_solve(..., if_first = 0) continues bit for bit as without it, also
 * behind a foreign point.  It works on any initialised solver (before, after and between solves, after cuadmm_update_bC / _update_A,
 * with any option) and on every plan of the engine: A X is formed from the engine's whole A by the iteration's kernel.  Device memory
 * beyond the auxiliary projector of cuadmm_lower_bound: at most 3 vec_len + con_num doubles (con_num more where the y-solve runs on the
 * host) and the per-block lists, allocated on first use and kept (cuadmm_get_evaluate_info).
 * CUADMM_ERR_INVALID, with the solver as it was: not initialised, out16 NULL, world > 1 or an in-process group (its sums are not
 * all-reduced), a passed vector with an entry that is not finite (checked on the host before anything is uploaded), no svec slots.
 * CUADMM_ERR_EIG: a block projection reported failure.  CUADMM_ERR_FACTOR: behind a failed cuadmm_update_A. */
int cuadmm_evaluate(cuadmm_solver* s, const double* X, const double* y, const double* S, double out16[16], double* per_block);
/* [0] calls of cuadmm_evaluate so far, [1] bytes of device memory the evaluation holds beyond the auxiliary projector (exact), [2] the
 * auxiliary projector's bytes (its vectors exactly, plus an estimate of its plan; shared with the lower bound and the infeasibility
 * check), [3] milliseconds of device time of the last call. */
int cuadmm_get_evaluate_info(const cuadmm_solver* s, double out4[4]);
/* Certified lower bounds on the smallest eigenvalue of every PSD block of X (which = 0), S (1) or S^ = C - A'y at the y cuadmm_get_y
 * would return (2; formed as cuadmm_lower_bound forms it), by bisection on the shift mu of a floating-point Cholesky factorisation of
 * M_k + mu I ("Certified lambda_min").  A factorisation that runs to completion proves lambda_min(M_k) >= -mu - margin (Higham,
 * Accuracy and Stability of Numerical Algorithms, Thm 10.3; margin: cuadmm_lambda_min_margin), so lo_k is CERTIFIED; hi_k = -(the largest
 * shift that failed) is an estimate and is NOT certified.  steps (1 .. 40): bisection steps; with T steps lo_k lies within the factor
 * (nu_max / nu_floor)^(2^-T) of the smallest shift that can succeed, 12 gives about 1 %.  Results in the caller's units: behind a solve the
 * scaled iterate is read where it lies and the numbers are rescaled (lo rounded down); the deferred unscaling is not triggered and nothing
 * the iteration reads changes: a following cuadmm_solve(..., if_first = 0) continues bit for bit.
 * out8: [0] min_k lo_k over the PSD blocks, [1] its block (-1: there is none), [2] max(0, -[0]) / (1 + ||b||) for which = 0,
 * / (1 + ||C||) for which = 1, 2: DIMACS err2 / err4 as DIMACS defines them, bounded from above, [3] which = 2 with trace bounds set
 * (cuadmm_set_trace_bounds): LB_lambda = b'y - sum_k R_k nubar_k with nubar_k = max(0, -lo_k) on PSD blocks and ||s^_k||_2 on
 * unconstrained ones, never below cuadmm_lower_bound's value up to rounding; otherwise NaN, [4] blocks with flag 3, [5] blocks with flag 1,
 * [6] milliseconds of device time (HIP events), [7] bytes of device memory held (allocated on first use and kept; the auxiliary
 * projector's vectors included).  per_block (may be NULL): 3 mat_num doubles, [3k] lo_k, [3k + 1] hi_k, [3k + 2] flag: 0 refined,
 * 1 PSD at the floor (the factorisation succeeded at the smallest shift tried, nu_floor = (n + 2) 2^-52 ||M_k||_F; hi_k = min_i m_ii),
 * 2 unconstrained block (lo = hi = 0), 3 unrefined: n > 1024 or max |m_ij| outside [2^-500, 2^500]: no factorisation, lo_k = -nu_max
 * from Gershgorin's discs, hi_k = min_i m_ii.
 * CUADMM_ERR_INVALID, with the solver as it was: not initialised, out8 NULL, world > 1 or an in-process group, which outside 0 .. 2,
 * steps outside 1 .. 40.  CUADMM_ERR_FACTOR: which = 2 behind a failed cuadmm_update_A. */
int cuadmm_lambda_min(cuadmm_solver* s, int which, int steps, double out8[8], double* per_block);
/* (n + 2) 2^-52 (trace + n mu): the margin of a factorisation of M + mu I that succeeded, trace = tr M.  Host only. */
double cuadmm_lambda_min_margin(int n, double trace, double mu);
/* Numerical rank and a low-rank factor M_k ~ L_k L_k' of every PSD block of X (which = 0) or S (1), by Cholesky with diagonal (complete)
 * pivoting in its lazy left-looking form ("Low-rank factors"; csrc/lowrank.hip): with d the residual diagonal, d_i = m_ii at
 * the start, column r takes the pivot p_r = argmax_i d_i over the rows not yet chosen (ties: the smallest index) while d_p > thr =
 * tol max(max_i m_ii, 0) and r < min(n_k, rmax); L[p, r] = sqrt(d_p), L[i, r] = (m_ip - sum_{j<r} L[i, j] L[p, j]) / L[p, r],
 * d_i <- d_i - L[i, r]^2.  The Schur complement is never formed: O(n r) scratch and O(n r^2) work for rank r, any block size the engine
 * accepts.  No eigenvalue is computed.  tol: relative, 0 <= tol < 1.  rmax: 1 .. 8192, the column cap.
 * What the factor promises, with E = M - L L', r the rank reported and u = 2^-53:
 *   structure          L[piv[j], j] > 0; L[piv[i], j] == 0.0 exactly for i < j; columns >= r are zero.
 *   residual diagonal  |E_ii - d_i| <= 2 (r + 2) u (m_ii + sum_j L_ij^2) for every row, d_i = 0 on pivot rows; resid is sum |d_i| of the
 *                      computed values over the rows not chosen.
 *   PSD input          for M >= 0, E >= 0 in exact arithmetic and ||E||_F <= tr E; in floating point ||M - L L'||_F <= resid +
 *                      4 (n + 2) u tr M.
 *   rank               after r columns max_i d_i >= tr E / n >= lambda_{r+1}(M) / n: a block of exact rank r0 (up to n u ||M|| << tol
 *                      max_i m_ii) with lambda_{r0}(M) / n > tol max_i m_ii is reported with rank exactly r0.
 * Results in the caller's units: behind a solve the scaled iterate is read where it lies and the numbers are rescaled (L by the root of
 * the scale, resid, dneg and the trace by the scale); the deferred unscaling is not triggered and nothing the iteration reads changes: a
 * following cuadmm_solve(..., if_first = 0) continues bit for bit.  A is not read: a failed cuadmm_update_A does not block the call.
 * out8: [0] sum_k r_k, [1] max_k r_k, [2] its block (the first; -1: there is no PSD block), [3] sum_k resid_k, [4] min_k dneg_k,
 * [5] blocks with flag 1, [6] milliseconds of device time (HIP events), [7] bytes of device memory held (lists and buffers, allocated on
 * first use, regrown when rmax grows, kept).
 * per_block (may be NULL): 6 mat_num doubles, [6k] rank r_k, [6k + 1] resid_k, [6k + 2] dneg_k = min(0, min_i d_i) over the rows not
 * chosen (negative: the block is not PSD), [6k + 3] tr M_k, [6k + 4] flag: 0 complete (every remaining d_i <= thr), 1 stopped at the
 * column cap with some d_i > thr, 2 unconstrained block (rank 0 and nothing else), 3 not factored: an entry is not finite or max |m_ij|
 * lies outside [2^-500, 2^500] (rank 0, resid NaN), [6k + 5] offset of the block's factor in L_out, in doubles.
 * L_out (may be NULL): cuadmm_lowrank_size doubles; block k holds n_k min(n_k, rmax) of them at its offset, column by column, n_k
 * doubles per column in the block's row order, columns >= r_k zero.  piv_out (may be NULL): as many ints; block k's min(n_k, rmax)
 * pivots stand at the same offset, -1 beyond r_k and everywhere else.
 * CUADMM_ERR_INVALID, with the solver as it was: not initialised, out8 NULL, world > 1 or an in-process group, which outside 0 .. 1,
 * tol not in [0, 1), rmax outside 1 .. 8192. */
int cuadmm_lowrank(cuadmm_solver* s, int which, double tol, int rmax, double out8[8], double* per_block, double* L_out, int* piv_out);
/* doubles of L_out (and ints of piv_out) that cuadmm_lowrank writes for this rmax: sum over the PSD blocks of n_k min(n_k, rmax).  Host only. */
int cuadmm_lowrank_size(const cuadmm_solver* s, int rmax, long long* count_out);
/* Trace bounds read off the constraints (the arrays of cuadmm_init).  R_out[k] = -1: nothing found (always for unconstrained blocks).
 * Rule 1: a constraint whose entries are exactly the diagonal slots of ONE PSD block, all with the same value c (c svec(I_k)), gives
 * tr X_k = b_j / c.  Rule 2: a block whose every diagonal entry is fixed by a constraint with that single entry has the sum of those
 * values as its trace.  The smaller one where both fire; a negative right-hand side: that rule finds nothing.  Host only (no device needed). */
int cuadmm_trace_bounds_detect(int vec_len, int con_num, const int* At_csc_col_ptrs, const int* At_csc_row_ids, const double* At_csc_vals,
                               const int* b_indices, const double* b_vals, int b_nnz, const int* blk_vals, int mat_num, double* R_out);
/* The in-process group a handle leads after cuadmm_duo_init(device_num_requested = N) from one process (reference
 * src/duo_solver.cu:487-577): [0] engines in the group (1: no group), [1] exchange of its all-reduce -- 1 = device side (each
 * rank's kernel adds the N staging buffers out of its peers' memory: one shared device, or peer access over xGMI as
 * src/utils/check_gpus.cu:29-43), 0 = host-staged fallback --, [2] distinct devices, [3] all-reduces so far. */
int cuadmm_get_group_info(const cuadmm_solver* s, double out4[4]);

/* ------------------------------------------------------------------------------------ */
/* TXT problem loader: Problem::from_txt (reference src/problem.cu:11-83, src/utils/io.cu). */
/* ------------------------------------------------------------------------------------ */
typedef struct cuadmm_problem cuadmm_problem;
typedef struct {
  int vec_len, con_num, mat_num;
  int At_nnz, b_nnz, C_nnz;
  const int* At_csc_col_ptrs;
  const int* At_csc_row_ids;
  const double* At_csc_vals;
  const int* b_indices;
  const double* b_vals;
  const int* C_indices;
  const double* C_vals;
  const int* blk_vals;
} cuadmm_problem_view;

/* prefix must end in '/' exactly like the reference CLI (problem.cu:12 concatenates) */
int cuadmm_problem_from_txt(const char* prefix, cuadmm_problem** out);
int cuadmm_problem_view_get(const cuadmm_problem* p, cuadmm_problem_view* view);
void cuadmm_problem_free(cuadmm_problem* p);
/* COO_to_CSC (io.cu:187-243): sorts triplets by (col,row) in place and fills col_ptrs[col_num+1] */
int cuadmm_coo_to_csc(int* col_ptrs, int* col_ids, int* row_ids, double* vals, int nnz, int col_num);
/* read_blk (io.cu:296-329): returns number of entries; types[i] in 'a'..'z','A'..'Z' */
int cuadmm_read_blk(const char* filename, char* types, int* sizes, int cap);
/* a sparse vector file (b.txt / C.txt: lines "idx 0 value"): returns the number of entries in the file and fills the first cap of them */
int cuadmm_read_sparse_vec_txt(const char* filename, int* indices, double* vals, int cap);
/* DeviceDenseVector::to_txt format (memory.h:278-294): one "%.32f\n" per entry */
int cuadmm_write_dense_txt(const char* filename, const double* vals, int64_t n);

/* ------------------------------------------------------------------------------------ */
/* Block bookkeeping (host): analyze_blk / is_large_mat / MatrixSizes / get_maps.          */
/* ------------------------------------------------------------------------------------ */
/* is_large_mat (src/matrix_sizes.cu:14-19) */
int cuadmm_is_large_mat(int mat_size, int mat_num);
/* analyze_blk (src/utils/analyze_blk.cu:63-99): ascending unique sizes + counts; returns #sizes */
int cuadmm_analyze_blk(const int* blk, int mat_num, int* sizes_out, int* nums_out, int cap);
/* get_maps (src/utils/get_maps.cu:80-135): the reference's int32 svec->dense maps.  The
 * engine itself computes indices from (offset,n) per block; these are exported so that the
 * svec index contract can be checked bit-for-bit against the reference's test vectors. */
int cuadmm_get_maps(const int* blk, int mat_num, int vec_len, int* map_B, int* map_M1, int* map_M2);
/* get_maps_duo (get_maps.cu:21-68) */
int cuadmm_get_maps_duo(const int* blk, int mat_num, int LARGE, int SMALL, int vec_len,
                        int* map_B, int* map_M1, int* map_M2);
/* get_inverse_permutation (src/utils/inverse_permutation.cu:17-30) */
int cuadmm_inverse_permutation(const int* perm, int n, int* perm_inv);
/* contiguous block ranges per rank balanced by sum n^3; out has world+1 entries */
int cuadmm_partition_blocks(const int* blk, int mat_num, int world, int* first_block_out);
/* Rows of the dense GPU tail of the replicated y-solve (k columns, padded to K = a multiple of 64) that rank p of `world` applies
 * when the tail is sharded (option "tail_shard"; the reference splits its per-iteration heavy part over the devices,
 * src/duo_solver.cu:269-295): [out[p], out[p + 1]) in the kernels' numbering (row 0 = the longest row of the triangle), equal shares
 * of the triangle's ENTRIES, multiples of 8, out[0] = 0, out[world] = K; a range may be empty.  Host arithmetic only. */
int cuadmm_tail_shard_bounds(int k, int world, int* out);

/* ------------------------------------------------------------------------------------ */
/* Host (A A^T + eps I) factor + permuted solve: CholeskySolverCPU                        */
/* (reference include/cuadmm/cholesky_cpu.h:62-155; CHOLMOD simplicial LDL^T there).      */
/* ------------------------------------------------------------------------------------ */
typedef struct cuadmm_aat cuadmm_aat;
/* A is given in CSC (col_ptrs over the vec_len columns = the reference's At_csr arrays,
 * solver.cu:91-95).  Factors P (A A^T + eps I) P^T = L D L^T with a fill-reducing P. */
int cuadmm_aat_create(int con_num, int vec_len, const int* A_col_ptrs, const int* A_row_ids,
                      const double* A_vals, double eps, cuadmm_aat** out);
/* CHOLMOD L->Perm semantics: row i of the permuted system is original row perm[i] */
const int* cuadmm_aat_perm(const cuadmm_aat* f);
int64_t cuadmm_aat_factor_nnz(const cuadmm_aat* f);
/* column pointers (m+1) of the strict lower triangle of L, for diagnostics */
const int64_t* cuadmm_aat_factor_colptr(const cuadmm_aat* f);
/* cholmod_solve2(CHOLMOD_LDLt): NO permutation applied inside (cholesky_cpu.h:146-155);
 * caller does rhs_perm[perm_inv[i]] = rhs[i] and y[perm[i]] = sol_perm[i] (solver.cu:487,500) */
int cuadmm_aat_solve_permuted(const cuadmm_aat* f, const double* rhs_perm, double* sol_perm);
/* Dense-tail split of the solve (no reference counterpart: CHOLMOD runs both sweeps on the host).  The last k
 * columns of L are an almost dense triangle holding most of nnz(L); the engine inverts that triangle once on the GPU
 * and runs it as two GEMVs per solve, the host keeps the sparse leading columns.
 *   tail_plan            : k chosen by the cost model (0 = keep everything on the host), k <= max_k
 *   tail_dense           : trailing k x k block of L as dense row-major unit-lower matrix (leading dimension ld) and D
 *   solve_leading_forward: forward sweep over the leading m-k columns, in place; x[m-k..] then holds z2
 *   solve_leading_backward: D1^-1 and backward sweep over the leading columns, in place; x[m-k..] must hold the solved tail */
int cuadmm_aat_tail_plan(const cuadmm_aat* f, int max_k);
/* Split factorisation: like cuadmm_aat_create, but when the cost model finds a dense tail (k <= max_k) the last k
 * columns are left unfactored; the Schur complement B22 - L21 D1 L21^T (sparse, lower triangle) is kept for the
 * GPU, which scatters it into a dense matrix, factors and inverts it (tail_solve.hip).
 * max_k < 0 forces the tail size -max_k.  cuadmm_aat_solve_permuted / _tail_dense are unavailable on a split factor. */
int cuadmm_aat_create_split(int con_num, int vec_len, const int* A_col_ptrs, const int* A_row_ids,
                            const double* A_vals, double eps, int max_k, cuadmm_aat** out);
int cuadmm_aat_tail_k(const cuadmm_aat* f);
/* > 0: the cost model chose this tail for the device-side solve with DENSE TREE TOPS -- the leading elimination forest cut at this
 * height, the nodes above it solved through explicit inverses of their diagonal blocks (engine option "lead_tops") --; 0 otherwise.
 * cuadmm_aat_plan_allow_tops(0) makes the calling thread's next cuadmm_aat_create_split plan without them (the planner of round 4). */
int cuadmm_aat_tail_tops(const cuadmm_aat* f);
void cuadmm_aat_plan_allow_tops(int allow);
/* Whole (unsplit) factor for a device-side solve: the strict lower triangle of the unit factor L by columns (Lp[m+1], Li, Lx),
 * the pivots D[m], and the elimination forest as lists of columns per tree (tree t: tree_cols[tree_ptr[t] .. tree_ptr[t+1]),
 * ascending).  The sweeps of a solve never leave a tree, so a block-diagonal A A^T (one small tree per group of coupled
 * constraints) is solved by one GPU thread per tree (engine: forest solve) in the arithmetic order of the host sweeps. */
int cuadmm_aat_factor_arrays(const cuadmm_aat* f, const int64_t** Lp, const int** Li, const double** Lx, const double** D);
int cuadmm_aat_forest(cuadmm_aat* f, int* n_trees, int* max_cols, const int** tree_ptr, const int** tree_cols);
/* lower triangle with diagonal of the Schur complement by rows (CSR over the k tail rows, tail-local column indices,
 * not sorted within a row); pointers stay valid until _tail_schur_release / _free */
int cuadmm_aat_tail_schur(const cuadmm_aat* f, const int64_t** row_ptr, const int** col, const double** val);
void cuadmm_aat_tail_schur_release(cuadmm_aat* f);
int cuadmm_aat_tail_dense(const cuadmm_aat* f, int k, double* L22, int64_t ld, double* D2);
/* (the leading sweeps of ONE factor are single-caller: they share per-factor scratch; different factors are independent) */
int cuadmm_aat_solve_leading_forward(const cuadmm_aat* f, int k, double* x);
int cuadmm_aat_solve_leading_backward(const cuadmm_aat* f, int k, double* x);
/* The same sweeps restricted to L11 (rows and columns < m-k) of a SPLIT factor whose L21 the engine keeps on the GPU (hybrid solve:
 * deep leading forest, most leading nonzeros in the tail rows):
 *   forward11 : x1 <- L11^-1 x1, x[m-k..] untouched (the GPU forms z2 = x2 - L21 x1)
 *   backward11: x1 <- L11^-T (D1^-1 x1 - w), w = L21^T x2 (m-k doubles, from the GPU); x[m-k..] is not read */
int cuadmm_aat_solve_leading_forward11(const cuadmm_aat* f, int k, double* x);
int cuadmm_aat_solve_leading_backward11(const cuadmm_aat* f, int k, double* x, const double* w);
/* Numeric refactorisation on the analysis of an existing factor (one-piece or split): A_vals are new values of A on the pattern given
 * to cuadmm_aat_create / _create_split, in that order (cuadmm_aat_pattern_nnz of them).  Ordering, elimination tree, Lp / Li, tail cut
 * and tops plan stay; the values of A A^T, the leading columns and the Schur complement of the tail (recomputed also after
 * _tail_schur_release) come from the code a fresh create runs, in its arithmetic order: the result equals a fresh create bit for bit.
 * A non-finite value is refused before anything changes (CUADMM_ERR_INVALID).  A zero or non-finite pivot returns CUADMM_ERR_FACTOR and
 * leaves a factor without usable values (cuadmm_aat_valid = 0) that a later successful refactorisation restores.  Single caller per
 * factor, like the sweeps. */
int cuadmm_aat_refactor(cuadmm_aat* f, const double* A_vals);
int cuadmm_aat_valid(const cuadmm_aat* f);
int64_t cuadmm_aat_pattern_nnz(const cuadmm_aat* f);
void cuadmm_aat_free(cuadmm_aat* f);

/* ------------------------------------------------------------------------------------ */
/* MATLAB front end (reference MATLAB/cuadmm_MATLAB.cu): the marshalled call behind            */
/*   [X, y, S, info] = cuadmm_MATLAB(eig_stream_num_per_gpu, max_iter, stop_tol, At, b, C, blk, X0, y0, S0, sig, ...)  */
/* Arguments are what mexFunction extracts from its mxArrays (cuadmm_MATLAB.cu:197-293): At as a sparse    */
/* vec_len x con_num matrix (size_t jc[At_cols+1], ir[nnz], pr[nnz]); b, C as sparse column vectors       */
/* (jc[2], ir, pr); blk as doubles; X0, y0, S0 dense; `optional5` = {sig_update_threshold, stage_1,        */
/* stage_2, switch_admm, sigscale} or NULL, read only under the reference's own conditions `nlhs >= 12..16`  */
/* (:297-333; nlhs <= 4, so the effective values are always 500, 50, 100, 11000 and sigscale 1.0).            */
/* The shim that calls this from a mexFunction: MATLAB/cuadmm_MATLAB_amd.cpp.                                  */
/* ------------------------------------------------------------------------------------ */
typedef struct cuadmm_mex_result cuadmm_mex_result;
int cuadmm_mex_call(int eig_stream_num_per_gpu, int max_iter, double stop_tol,
                    size_t At_rows, size_t At_cols, const size_t* At_jc, const size_t* At_ir, const double* At_pr,
                    size_t b_rows, const size_t* b_jc, const size_t* b_ir, const double* b_pr,
                    size_t C_rows, const size_t* C_jc, const size_t* C_ir, const double* C_pr,
                    size_t blk_len, const double* blk_pr,
                    size_t X0_len, const double* X0, size_t y0_len, const double* y0, size_t S0_len, const double* S0,
                    double sig, int nlhs, const double* optional5, cuadmm_mex_result** out);
/* what the MEX packs into its outputs (cuadmm_MATLAB.cu:366-424): X, y, S (unscaled) and the 10 x 2 `info` cell:
 * iter_num, the eight per-iteration arrays (which = CUADMM_INFO_*, iter_num doubles each) and total_time */
int cuadmm_mex_result_dims(const cuadmm_mex_result* r, int* vec_len, int* con_num, int* iter_num, double* total_time);
int cuadmm_mex_result_XyS(const cuadmm_mex_result* r, double* X, double* y, double* S);
int cuadmm_mex_result_info(const cuadmm_mex_result* r, int which, double* out);
void cuadmm_mex_result_free(cuadmm_mex_result* r);

/* ------------------------------------------------------------------------------------ */
/* Op-level device entry points (pointers are DEVICE pointers; `stream` is a hipStream_t   */
/* or NULL).  Each mirrors one reference kernel/wrapper so parity can be tested per op.    */
/* ------------------------------------------------------------------------------------ */
/* vector_to_matrices / matrices_to_vector (src/kernels/vec_mat_conversion.cu:11-98) */
int cuadmm_op_vector_to_matrices(const double* Xb, double* large_mat, double* small_mat,
                                 const int* map_B, const int* map_M1, const int* map_M2,
                                 int vec_len, void* stream);
int cuadmm_op_matrices_to_vector(double* Xb, const double* large_mat, const double* small_mat,
                                 const int* map_B, const int* map_M1, const int* map_M2,
                                 int vec_len, void* stream);
/* batch_eig_cusolver / single_eig_cusolver (include/cuadmm/cusolver.h:76-95,154-171):
 * `count` contiguous n x n column-major symmetric matrices, overwritten by eigenvectors
 * (column-major, column k <-> W[k]); W ascending; info[i] = 0 or 1 (iteration cap hit / orthonormalisation not converged).
 * n <= 128: one wavefront / workgroup per matrix; 129 <= n <= 8192: one matrix at a time on the whole chip (csrc/eig_large.hip:
 * tridiagonalisation, bisection, inverse iteration, Cholesky-QR; n = 2000 in 0.06 s); larger n: CUADMM_ERR_INVALID. */
int cuadmm_op_batch_eig(double* mat, double* W, int* info, int n, int count, void* stream);
/* The DGEMM of the large-block rebuild (the reference calls cublasDgemm on large_mat, src/solver.cu:630-644).
 * C = alpha * A * B + beta * E for n x n row-major SYMMETRIC A and B (device pointers, n a multiple of 64,
 * E may be null); this is the fp64 matrix-core kernel behind the large-block projection (psd_large.hip). */
int cuadmm_op_gemm_sym(int n, const double* A, const double* B, double alpha, double beta, const double* E,
                       double* C, void* stream);
/* The GPU part of the A*A^T solve on its own (tail_solve.hip): z <- L22^-T D2^-1 L22^-1 z for `nrhs` host vectors
 * of length k (contiguous), L22 dense k x k row-major unit lower triangular and D2 the pivots (host pointers). */
int cuadmm_op_tail_solve(const double* L22_host, const double* D2_host, int k, double* z2_host, int nrhs);
/* The same solve as the ranks of a sharded engine run it (TailSolve::shard_*): out_host receives `world` partial results of k doubles,
 * partial p = what rank p contributes from its rows [bounds[p], bounds[p + 1]) (cuadmm_tail_shard_bounds) -- their sum in rank order
 * is the solve; rows_out[p] = the rows rank p applied.  one_pass: bit 0 = the one-pass kernels (0: the two triangular GEMVs), bit 1 = every rank
 * keeps only its rows of inv(L22) (one object per rank, as the ranks of an engine do since round 6). */
int cuadmm_op_tail_solve_sharded(const double* L22_host, const double* D2_host, int k, const double* z_host, int world, int one_pass,
                                 double* out_host, int* rows_out);
/* Test hook: failure drill of the row-sharing tail kernel (18 432 < k <= 32 768).  out_host: 4 x k doubles -- the plain solve, the
 * solve of a right-hand side poisoned with a NaN that carries the exchange sentinel's bits, the solve with the lost-exchange
 * counter raised beforehand (NaN), the solve after the object retired to the two-pass kernels; counts[3] = {exchanges lost by the
 * poisoned solve (0), count found and cleared after the third solve (>= 1), retired flag (1)}. */
int cuadmm_op_tail_solve_drill(const double* L22_host, const double* D2_host, int k, const double* z_host, double* out_host, int* counts);
/* Test hook only: the device y-solve of a SPLIT factor (cuadmm_aat_create_split; its Schur complement not yet released) on its own: the GPU
 * tail and the leading sweeps built as the engine builds them, with the engine's switches of the sweeps -- stream_only (option "lead_stream"),
 * small_kb ("lead_small_kb"), tops_level ("lead_tops": -1 automatic, 0 never, L > 0 cut at height L), force_hybrid ("l21_device" = 2: host
 * sweeps over L11, L21 and the tail on the device).  What was built runs; the engine's cost model is not asked.  ax, asmc, b: nrhs x m host
 * doubles in the factor's order, y_out[r] = (L D L^T)^-1 (-asmc[r] + (b[r] - ax[r]) * isig), solved one after the other on the same objects.
 * info11 = {ntrees, max_levels, n_small, n_big, n_stream, n_micro, n_long, tops, nT, hybrid, ready}: which kernels served the forest. */
int cuadmm_op_lead_solve(const cuadmm_aat* f, int m, int stream_only, int small_kb, int tops_level, int force_hybrid, const double* ax,
                         const double* asmc, const double* b, double isig, int nrhs, double* y_out, int* info11);
/* Test hook only: the same solve by one GPU thread per tree of a ONE-PIECE factor's elimination forest (what the engine runs for a
 * block-diagonal A A^T); info2 = {trees, columns of the largest tree}. */
/* value pass of cuadmm_update_A: outA[offA + q] = src[fromA[q]] (q < nA), outAt[offAt + q] = src[fromAt[q]] (q < nAt) on device arrays of
 * nA + offA + 2 / nAt + offAt + 2 doubles filled with `fill` first and returned whole */
int cuadmm_op_gather_vals(const double* src, int n_src, const int* fromA, int nA, int offA, const int* fromAt, int nAt, int offAt, double fill,
                          double* outA, double* outAt);
int cuadmm_op_forest_solve(cuadmm_aat* f, int m, const double* ax, const double* asmc, const double* b, double isig, double* y_out, int* info2);
/* Test hooks only: the kernels of an ADMM iteration as ops.  Every pointer is a HOST pointer; in/out arrays are uploaded as given, so what a
 * kernel leaves untouched comes back bit for bit.
 *   aty_xb   : Rd1 = At y - C and, with write_xb, Xb = X + sig Rd1; At in CSR over the L svec rows (m columns); info2 = {long rows, longest short row}
 *   post     : mode 0 / 1 / 2 = the three update steps behind the projection (X, S in/out, sums2 = {sum Rd^2, <C, X>} in/out); mode 3 = the one-pass
 *              second half of an sGS iteration (takes At, y and m instead of Xproj and Rd1); *nparts_out = partial pairs the final reduction summed
 *   spmv_rows: outX = A X, outS = A (S - C) over the rows of A (CSR, ncols columns) where want_x / want_s; with rowmap (compact row -> slot of an
 *              out_len vector) the engine's compact-list variant, else out_len = rows; info4 = {lanes per row, long-row cap, long rows, segments}
 *   rp_stats : out4 = {sum (normA (b - ax) bscale)^2, b . y, sums2[0], sums2[1]} */
int cuadmm_op_aty_xb(int64_t L, int m, const int* row_ptrs, const int* col_ids, const double* vals, const double* y, const double* C, const double* X,
                     double sig, int write_xb, double* Rd1, double* Xb, int* info2);
int cuadmm_op_post(int mode, int64_t L, const double* Xproj, const double* Rd1, const double* C, double* X, double* S, double inv_sig, double tau_sig,
                   double* sums2, int m, const int* row_ptrs, const int* col_ids, const double* vals, const double* y, int* nparts_out);
/* The acceleration kernels on host arrays (csrc/accel.hip).  State vectors have 2 L entries, X part then S part.
 *   push:    g_out = (X - u_X, sig (S - u_S)); with have_prev also dF_out = (X - f_X, sig (S - f_S)) and dG_out = g - g_prev (else both are
 *            left as they were); f_prev is in / out and returns (X, S); gnorm2_out[0] = ||g||^2
 *   gram:    out[j] = <dG_newest, dG_j>, out[cols + j] = <dG_j, g>, j < cols; ring_dG holds cols columns of L2 entries (L2 even)
 *   combine: X <- X - sum_j gamma_j dF_j[X], S <- (sig S - sum_j gamma_j dF_j[S]) / sig; ring_dF holds cols columns of 2 L entries */
int cuadmm_op_accel_push(int64_t L, const double* u_prev, const double* X, const double* S, double sig, double* f_prev, const double* g_prev, int have_prev,
                         double* g_out, double* dF_out, double* dG_out, double* gnorm2_out);
int cuadmm_op_accel_gram(int64_t L2, int cols, int newest, const double* ring_dG, const double* g, double* out /* 2 cols */);
int cuadmm_op_accel_combine(int64_t L, int cols, const double* ring_dF, const double* gamma, double sig, double* X_inout, double* S_inout);
/* The roll kernel of the infeasibility check on host arrays (csrc/infeas.hip): d = cur - prev, prev_inout <- cur, d_out = d (negate: -d;
 * 0 inside the nz ranges [zoff[r], zoff[r] + zlen[r])), sums2_out = [||d||^2, <w, d>].  offset = 1 places the device vectors one double
 * behind a 16-byte boundary (the kernel's one-double path), 0 on one (two doubles per access). */
int cuadmm_op_infeas_roll(int64_t n, const double* cur, double* prev_inout, const double* w, int negate, int nz, const int64_t* zoff, const int64_t* zlen,
                          int offset, double* d_out, double* sums2_out);
/* The per-block norm kernels of the lower bound on host arrays (csrc/lower_bound.hip): pairs_out[2k] = sum of M^2, [2k + 1] = sum of P^2
 * over the slots of block k (blk: sizes as in cuadmm_init; offs: first slot of every block in the n-vectors, NULL: one behind the other
 * from slot 0); comb3_out = [sum_k R_k nubar_k, the block with the largest term, that term] with nubar_k as in cuadmm_lower_bound on
 * sqrt(pairs).  offset = 1 places both vectors one double behind a 16-byte boundary, so that the one-double heads and tails run.  M and P
 * are copied back as the kernels left them. */
int cuadmm_op_lb_block_norms(int64_t n, double* M_inout, double* P_inout, int nblk, const int* blk, const int64_t* offs, const double* R, int offset,
                             double* pairs_out, double* comb3_out);
/* The per-block statistics kernels of cuadmm_evaluate on host arrays (csrc/evaluate.hip): sums6_out[6k + ...] = sum X^2, sum (PX - X)^2,
 * sum S^2, sum (PS - S)^2, sum X S, sum (Rd1 + S)^2 over the slots of block k; an unconstrained block (negative size) has 0 and sum S^2
 * as its second and fourth.  blk, offs, offset as in cuadmm_op_lb_block_norms; every block's size and range is checked before anything
 * is launched.  The five vectors are copied back as the kernels left them (they write none of them). */
int cuadmm_op_ev_block_stats(int64_t n, double* X_inout, double* S_inout, double* PX_inout, double* PS_inout, double* Rd1_inout, int nblk, const int* blk,
                             const int64_t* offs, int offset, double* sums6_out /* 6 nblk */);
/* The kernel of cuadmm_lambda_min on a DEVICE svec vector whose blocks follow one another from slot 0 (csrc/lambda_min.hip); blk_vals on
 * the host (negative: unconstrained).  per_block3_host: 3 mat_num doubles, lo, hi, flag per block as in cuadmm_lambda_min.  Synchronises
 * the stream. */
int cuadmm_op_block_lambda_min(const double* svec_dev, const int* blk_vals, int mat_num, int steps, double* per_block3_host, void* stream);
/* The kernel of cuadmm_lowrank on a DEVICE svec vector whose blocks follow one another from slot 0 (csrc/lowrank.hip); blk_vals on the
 * host (negative: unconstrained).  per_block6_host: 6 mat_num doubles; L_host, piv_host (each may be NULL): sum n_k min(n_k, rmax) doubles
 * and ints, all three laid out as in cuadmm_lowrank.  Synchronises the stream. */
int cuadmm_op_block_lowrank(const double* svec_dev, const int* blk_vals, int mat_num, double tol, int rmax, double* per_block6_host, double* L_host,
                            int* piv_host, void* stream);
/* The kernel of cuadmm_set_lowrank on a DEVICE svec vector whose blocks follow one another from slot 0 (csrc/lowrank_apply.hip): every
 * slot of every PSD block is written, the slots of unconstrained blocks (blk_vals negative) keep their bits.  L_host (NULL where every
 * rank is 0), ranks and blk_vals on the host, L_host laid out as in cuadmm_set_lowrank.  Synchronises the stream. */
int cuadmm_op_block_outer(const double* L_host, const int* ranks, const int* blk_vals, int mat_num, int rmax, double* svec_dev_inout, void* stream);
/* The host side of that kernel.  loff_out (may be NULL): mat_num + 1 offsets of the blocks' factors for rmax.  tasks_out (may be NULL): up
 * to cap_slots wavefront slots of four ints (block or -1, first tile, end, step) over the tiles of the block's lower triangle numbered
 * row by row; four consecutive slots are one workgroup.  split_from: the size from which a block is split over workgroups (0: the
 * engine's; at least 33).  Returns the number of slots, or an error.  Host only (no device needed). */
int cuadmm_op_block_outer_plan(const int* blk_vals, int mat_num, int rmax, int split_from, long long* loff_out, int* tasks_out, int cap_slots);
/* The kernel of cuadmm_block_multiply on a DEVICE svec vector whose blocks follow one another from slot 0 (csrc/block_mult.hip): W_host <-
 * sign * M_k V_k per PSD block (sign = 1 or -1), +0.0 in the columns >= ranks[k]; the vector is only read.  V_host (NULL where every rank
 * is 0) and W_host are laid out as in cuadmm_block_multiply for rmax; ranks and blk_vals on the host.  Synchronises the stream. */
int cuadmm_op_block_mult(const double* svec_dev, const int* blk_vals, int mat_num, double sign, const double* V_host, const int* ranks, int rmax, double* W_host,
                         void* stream);
/* The host side of that kernel.  loff_out (may be NULL): mat_num + 1 offsets of the blocks' V_k / W_k for rmax.  tasks_out (may be NULL):
 * up to cap_slots wavefront slots of two ints (block or -1, panel of 16 rows); four consecutive slots are one workgroup and hold panels
 * of one block, or blocks of one panel.  Returns the number of slots, or an error.  Host only (no device needed). */
int cuadmm_op_block_mult_plan(const int* blk_vals, int mat_num, int rmax, long long* loff_out, int* tasks_out, int cap_slots);
/* The multiplier pass of cuadmm_lowrank_grad alone (csrc/lowrank_grad.hip) on host arrays of m >= 1 doubles in the engine's scaled space
 * and order: rs_i = ax_i - b_i, r_out_i = (normA_i rs_i) bscale, ytilde_out_i = y_i - ((sigma r_out_i) normA_i) fl(1 / Cscale) (sigma = 0:
 * the bits of y_i), out2 = [bscale Cscale sum y_i rs_i, sum r_out_i^2] from 256 slot partials added in slot order.  Every operation is
 * rounded once.  The default stream, synchronised. */
int cuadmm_op_lrg_multiplier(int m, const double* ax, const double* b, const double* normA, const double* y, double bscale, double Cscale, double sigma,
                             double* ytilde_out, double* r_out, double out2[2]);
/* The outer-product kernel of cuadmm_lowrank_line on three DEVICE svec vectors whose blocks follow one another from slot 0
 * (csrc/lowrank_line.hip): x0 <- svec(L_k L_k'), x1 <- svec(L_k D_k' + D_k L_k'), x2 <- svec(D_k D_k') on every PSD block; the slots of
 * unconstrained blocks keep their bits.  L_host, D_host (one layout, cuadmm_lowrank's L_out for rmax), ranks and blk_vals on the host.
 * split_from as in cuadmm_op_block_outer_plan, whose task list this launch walks (0: the engine's; else at least 33).  Synchronises the
 * stream. */
int cuadmm_op_block_outer3(const double* L_host, const double* D_host, const int* ranks, const int* blk_vals, int mat_num, int rmax, int split_from,
                           double* x0_dev_inout, double* x1_dev_inout, double* x2_dev_inout, void* stream);
/* The streaming pass of cuadmm_lowrank_line alone (csrc/lowrank_line.hip) on host arrays of m >= 1 doubles in the engine's scaled space
 * and order: rs0_i = ax0_i - b_i, r_out_i = (normA_i rs0_i) bscale, p_out_i = (normA_i ax1_i) bscale, q_out_i = (normA_i ax2_i) bscale,
 * out9 = [u sum y rs0, u sum y ax1, u sum y ax2 (u = bscale Cscale), sum r^2, sum r p, sum p^2, sum r q, sum p q, sum q^2], each from
 * 256 slot partials added in slot order.  Every operation is rounded once.  A device vector starts in the 16-byte phase its host
 * array has: arrays that are all 16-byte aligned take the two-constraint map, any other the one-constraint map.  The default stream,
 * synchronised. */
int cuadmm_op_lrl_sums(int m, const double* ax0, const double* ax1, const double* ax2, const double* b, const double* normA, const double* y, double bscale,
                       double Cscale, double* r_out, double* p_out, double* q_out, double out9[9]);
/* The three streaming kernels of cuadmm_lowrank_refine alone (csrc/lowrank_refine.hip) on host arrays of n >= 1 doubles; G[e] =
 * 2.0 * (W[e] * unit) throughout, every operation rounded once.  A device vector starts in the 16-byte phase its host array has: arrays
 * that are all 16-byte aligned take the two-entry map, any other the one-entry map.  An array that is written has n + 1 doubles: entry n
 * travels to the device and back and comes back with its bits.  The default stream, synchronised.
 * lrr_dots: out3 = [sum G^2, sum G G_old, sum G D_old], each from 256 slot partials added in slot order.
 * lrr_direction: D[e] = fl(fl(beta D[e]) - G[e]), or - G[e] where restart != 0 (D is then not read); Ds[e] = fl(D[e] root); G_old[e] = G[e].
 * lrr_step: L[e] = fl(L[e] + fl(t D[e])); Ls[e] = fl(L[e] root). */
int cuadmm_op_lrr_dots(long long n, const double* W, double unit, const double* G_old, const double* D_old, double out3[3]);
int cuadmm_op_lrr_direction(long long n, const double* W, double unit, double beta, int restart, double root, double* D_inout, double* Ds_out, double* Gold_out);
int cuadmm_op_lrr_step(long long n, double t, double root, const double* D, double* L_inout, double* Ls_out);
/* The check of a caller's factors that cuadmm_set_lowrank, cuadmm_block_multiply, cuadmm_lowrank_grad, cuadmm_lowrank_line and
 * cuadmm_lowrank_refine share (csrc/factor_layout.h), alone: who is one of "set_lowrank", "block_multiply", "lowrank_grad", "lowrank_line",
 * "lowrank_refine" and words the message as
 * that call does; L is its factor buffer (V for block_multiply), D the second one of lowrank_line (not looked at for the others).
 * Returns what that call would return for these factors: 0, or CUADMM_ERR_INVALID with the message set.  Host only (no device needed). */
int cuadmm_op_check_factors(const char* who, const int* blk_vals, int mat_num, const int* ranks, int rmax, const double* L, const double* D);
int cuadmm_op_spmv_rows(int rows, int ncols, const int* row_ptrs, const int* col_ids, const double* vals, const double* X, const double* S, const double* C,
                        int want_x, int want_s, const int* rowmap, int out_len, double* outX, double* outS, int* info4);
int cuadmm_op_rp_stats(int m, const double* ax, const double* b, const double* normA, const double* y, double bscale, const double* sums2, double* out4);
/* Test hooks only: the fused step's list kernels, the quad sums, the copies and the update passes as ops (csrc/vec_kernels.hip).  Host
 * pointers; every index and length is checked before anything is launched; in/out arrays are uploaded as given, so what a kernel leaves
 * untouched comes back bit for bit; the default stream, synchronised.
 *   aty_xb_idx : Rd1[i] = (At y)[i] - C[i], Xb[i] = X[i] + sig Rd1[i] on the nidx rows i = idx[k] (each in [0, L)) only
 *   post_rest  : mode 0 / 1 of post over the rows of idx.  The partial array of 2 (nfused + post_grid(nidx)) doubles starts as fused_pairs
 *                followed by NaN and is returned whole in partials_out.  use_quads = 0: the launcher reduces into sums2 (mode 0);
 *                use_quads = 1: it reduces nothing and says in *nparts_out how many pairs there are (else *nparts_out = -1).
 *                nidx = 0 needs nfused > 0.
 *   reduce_quads: out4 = {sum p2.x, sum p2.y, sum p1.x, sum p1.y}, sums2 = out4[2..3] over n1 / n2 pairs; the device arrays hold pad_pairs
 *                NaN pairs behind the data; the segment scratch (with_scratch) starts as NaN; out4 and sums2 start as NaN and are copied
 *                back even where the launcher refuses (more than one segment without scratch: CUADMM_ERR_INVALID)
 *   reduce_quads_batch: p1, p2 hold iters x stride doubles (stride even, >= 2 n; iters in [1, 64]); out4 holds 4 iters + 4 doubles, uploaded
 *                as given: the last four are a canary
 *   closed_rows: nslots records whose every byte is 0xA5 except nk (1..8) and rows[0, nk) (each in [0, m)); cl_out (16 nslots, in/out) from
 *                closed_gather_out, then closed_patch_b; b_out[8 s + k] = rec[s].b[k]; *changed_out = record bytes outside b[0, nk) that
 *                differ from the upload
 *   copy       : dst_inout holds n + 4 doubles (4 canaries); scale: v_inout likewise
 *   copy_multi : count in [1, 6] jobs; dst_inout[q] holds nbytes[q] + 32 bytes
 *   update_svec: X, S and (may be NULL) C hold n + 2 doubles; update_cons: b, y (each may be NULL) hold m + 2; the launchers see n and m
 *   scatter_scaled: dst[idx[k]] = val[k] s; idx distinct and in [0, len) */
int cuadmm_op_aty_xb_idx(int64_t L, int m, const int* row_ptrs, const int* col_ids, const double* vals, const double* y, const double* C, const double* X,
                         double sig, int64_t nidx, const int* idx, double* Rd1_inout, double* Xb_inout);
int cuadmm_op_post_rest(int mode, int64_t L, int64_t nidx, const int* idx, int nfused, const double* fused_pairs, const double* Xproj, const double* Rd1,
                        const double* C, double* X_inout, double* S_inout, double inv_sig, double tau_sig, int use_quads, double* sums2_inout,
                        double* partials_out, int* nparts_out);
int cuadmm_op_reduce_quads(const double* p1, int n1, const double* p2, int n2, int pad_pairs, int with_scratch, double* out4, double* sums2);
int cuadmm_op_reduce_quads_batch(const double* p1, const double* p2, int n, int64_t stride, int iters, double* out4_inout);
int cuadmm_op_closed_rows(int nslots, const int* nk, const int* rows, int m, const double* ax, const double* as, const double* b, double* cl_out,
                          double* b_out, int64_t* changed_out);
int cuadmm_op_copy(const double* src, int64_t n, double* dst_inout);
int cuadmm_op_copy_multi(int count, const int64_t* nbytes, const void* const* src, void* const* dst_inout);
int cuadmm_op_scale(double* v_inout, int64_t n, double s);
int cuadmm_op_update_svec(int64_t n, double* X_inout, double* S_inout, double* C_inout, int zero, double x1, double x2, double s1, double s2);
int cuadmm_op_update_cons(int m, double* b_inout, double* y_inout, const double* normA, int ymode, double cs_old, double ics_new);
int cuadmm_op_scatter_scaled(int len, double* dst_inout, int n, const int* idx, const double* val, double s);
/* Same with the factorisation on the GPU too: z <- S^-1 z for a symmetric S given by its lower triangle with
 * diagonal (CSR over k rows, host pointers), dense LDL^T without pivoting (what cuadmm_aat_create_split hands over). */
int cuadmm_op_tail_factor_solve(const int64_t* row_ptr, const int* col, const double* val, int k, double* z_host, int nrhs);
/* max_dense_vector_zero (src/kernels/dense_scalar.cu:41-47,93-97) */
int cuadmm_op_max_zero(double* w, int64_t n, void* stream);
/* dense_matrix_mul_diag_batch (src/kernels/diagonal_batch.cu:11-62): out = in * diag(w) per matrix */
int cuadmm_op_mul_diag_batch(double* out, const double* in, const double* w, int n, int count, void* stream);
/* dense_matrix_mul_trans_batch (include/cuadmm/cublas.h:18-35): P = T * V^T per matrix (MFMA f64) */
int cuadmm_op_mul_trans_batch(double* P, const double* T, const double* V, int n, int count, void* stream);
/* fused PSD-cone projection over blocks laid out in svec form (solver.cu:534-647):
 * blk[mat_num] sizes in blk.txt order; Xproj may alias Xb.  eig_fail (device int, may be
 * NULL) is incremented per block whose QL iteration hit its cap. */
int cuadmm_op_psd_project(const double* Xb, double* Xproj, const int* blk_host, int mat_num, void* stream);
/* The same projection through a plan that is built once (block descriptors, size classes, workspaces on the device) and reused:
 * what the solver does every iteration; cuadmm_op_psd_project builds and drops a plan per call. */
typedef struct cuadmm_psd_plan cuadmm_psd_plan;
int cuadmm_psd_plan_create(const int* blk_host, int mat_num, int eig_rank, cuadmm_psd_plan** out);
int cuadmm_psd_plan_project(cuadmm_psd_plan* plan, const double* Xb, double* Xproj, int* steps_dev /* may be NULL */, void* stream);
void cuadmm_psd_plan_destroy(cuadmm_psd_plan* plan);
/* The plan in the state the engine keeps it in (test hooks).  set_hint: the schedule warm start, a caller-owned device array of mat_num
 * ints (lift steps of the previous projection, read and written by the sign kernels; aged every 16th projection), on the batched-GEMM
 * path for the groups padded to at most hint_max_n; NULL switches it off.  reorder: longest block first -- the members of the
 * one-wavefront classes re-sorted by steps_host[mat_num] (async: from a page-locked copy by a command queued on the stream).
 * project_ordered: the projection on the null stream (own_stream = 0) or on a non-blocking stream of the plan's (1: size classes fork
 * to side streams and join), a copy Xproj -> snap_dev (may be NULL) queued on that stream right behind it, and a synchronisation of
 * that stream only; *fails_out = the plan's cumulative count of blocks that hit an iteration cap. */
int cuadmm_psd_plan_set_hint(cuadmm_psd_plan* plan, int* hint_dev, int hint_max_n);
int cuadmm_psd_plan_reorder(cuadmm_psd_plan* plan, const int* steps_host, int async, int own_stream);
int cuadmm_psd_plan_project_ordered(cuadmm_psd_plan* plan, const double* Xb, double* Xproj, double* snap_dev /* may be NULL */, int* steps_dev /* may be NULL */,
                                    int own_stream, int* fails_out /* may be NULL */);
/* Test hook, host only (no device is touched): the launch ranges a plan of these blocks builds under the default options changed by
 * opt_keys[n_opts] = opt_vals[n_opts] ("psd_*").  ranges_out: 10 ints per range, at most 8 ranges, in launch order: size class,
 * first, count (members of ids_out), kind (0 register eigensolver, 1 workgroup eigensolver, 2 whole-chip eigensolver, 3 one-wavefront
 * sign, 4 one-workgroup sign), tiles of 16 per side, wavefronts per SIMD of single / batched launches, full, triple, largest member.
 * ids_out[mat_num]: the members (block ids); slot_out[mat_num]: partial-sum slot of the fused launches per block, -1: not fused;
 * rest_out[svec length]: svec elements outside the fused blocks.  summary_out[6]: ranges, members, rest elements, fusable,
 * fused blocks, first size on the batched-GEMM path. */
int cuadmm_psd_plan_ranges(const int* blk_host, int mat_num, int eig_rank, int tiny_sign, const char* const* opt_keys, const double* opt_vals,
                           int n_opts, int* ranges_out, int* ids_out, int* slot_out, int* rest_out, int* summary_out);
/* General form: blk[k] < 0 is an UNCONSTRAINED block of -blk[k] variables (blk.txt type 'u', reference README.md:55-64),
 * copied through; eig_rank > 0 keeps only the eig_rank largest eigenvalues of every PSD block: V diag(max(W,0) * mask) V^T with
 * the mask of get_eig_rank_mask.cu:13-37 (dense_scalar.cu:51-57) -- computed through the eigensolver kernels. */
int cuadmm_op_psd_project_ex(const double* Xb, double* Xproj, const int* blk_host, int mat_num, int eig_rank, int* steps_dev, void* stream);
/* Test hook: cuadmm_op_psd_project_ex on a plan whose options are the built-in defaults changed by opt_keys[n_opts] = opt_vals[n_opts]
 * ("psd_*"; an unknown key is an error).  The environment is NOT consulted, so no variable changes the kernel variant a test names. */
int cuadmm_op_psd_project_opts(const double* Xb, double* Xproj, const int* blk_host, int mat_num, int eig_rank, const char* const* opt_keys,
                               const double* opt_vals, int n_opts, int* steps_dev /* may be NULL */, void* stream);
/* Test hook, host only (no device is touched): the groups the batched-GEMM matrix-sign path forms of these blocks under the default
 * options changed by the pairs given -- the groups that share one launch first, then the others in the order they run.  out: 12 ints
 * per group, room for cap groups (more is an error; *n_groups_out is set either way): padded size N, members, merged (shares the
 * one launch of several padded sizes), slot, tile (32 | 64), tiles per member, decision kernel, one-launch kernel, spread (its
 * workgroups in plain order over the chip), grid of the one-launch kernel, super-block tile order (one member, >= 16 tiles per side),
 * fused (psd_lg_fuse and N <= 512: the one-launch kernel's own prologue and epilogue). */
int cuadmm_psd_sign_groups(const int* blk_host, int mat_num, const char* const* opt_keys, const double* opt_vals, int n_opts, int* out, int cap,
                           int* n_groups_out);
/* Same, also returning how many Newton-Schulz steps the adaptive matrix-sign schedule took per block (device int array of
 * mat_num entries, 0 for blocks served by the eigensolver kernels); developer/diagnostic entry. */
int cuadmm_op_psd_project_steps(const double* Xb, double* Xproj, const int* blk_host, int mat_num, int* steps_dev, void* stream);
/* Host model of the per-block adaptive schedule of the matrix-sign projection (csrc/sign_sched.h), no device needed:
 * s[n] = |eigenvalue| / ||X||_1 on entry, the sign estimates on exit; returns the number of steps the kernels would
 * take on that spectrum and, in *max_err_out, max_i s_i(0) |1 - s_i| / 2 (projection error relative to ||X||_1).
 * lagged: 0 = the one-wavefront / one-workgroup kernels (decisions from the current iterate), 1 = the batched-GEMM path
 * (||S - S Y|| one step old), 2 = every statistic one step old (measured and rejected), 3 = as 0 with the statistics passed
 * on every step (reference for the steps on which the kernels skip them); + 8: without the mega-lift of round 5 (sign_sched.h). */
int cuadmm_sign_sched_simulate(double* s, int n, int lagged, double* max_err_out);
/* same, with the schedule's warm start across ADMM iterations: lift0 = lift steps the previous projection of the block needed
 * (0: none), *lifts_out = the hint this run leaves */
int cuadmm_sign_sched_simulate_hint(double* s, int n, int lagged, int lift0, double* max_err_out, int* lifts_out);
/* perform_permutation (src/kernels/permutation.cu:12-33): v1[perm[i]] = v2[i] */
int cuadmm_op_permute(double* v1, const double* v2, const int* perm, int n, void* stream);
/* get_normA (src/kernels/sparse_matrix_norm.cu:11-44): per CSC column norm=max(1,||col||), col/=norm */
int cuadmm_op_get_normA(const int* col_ptrs, double* vals, double* normA, int con_num, void* stream);
/* SpMV_cusparse (include/cuadmm/cusparse.h:70-83): y = alpha*A*x + beta*y, CSR int32 */
int cuadmm_op_spmv_csr(int rows, const int* row_ptrs, const int* col_ids, const double* vals,
                       const double* x, double* y, double alpha, double beta, void* stream);
/* dense_dense.cu wrappers */
int cuadmm_op_axpby2(double* v1, const double* v2, double alpha, double beta, int64_t n, void* stream);           /* v1=a*v1+b*v2 (:92-100)  */
int cuadmm_op_axpby3(double* v1, const double* v2, const double* v3, double alpha, double beta, int64_t n, void* stream); /* v1=a*v2+b*v3 (:103-111) */
/* get_norm (include/cuadmm/memory.h:238-247): 2-norm, deterministic two-stage reduction */
int cuadmm_op_norm2(const double* v, int64_t n, double* host_out, void* stream);

/* device memory helpers for bindings that do not own a device allocator */
int cuadmm_dev_malloc(void** ptr, size_t bytes);
int cuadmm_dev_free(void* ptr);
int cuadmm_memcpy_h2d(void* dst, const void* src, size_t bytes);
int cuadmm_memcpy_d2h(void* dst, const void* src, size_t bytes);
int cuadmm_dev_sync(void);

#ifdef __cplusplus
}
#endif
#endif /* CUADMM_AMD_H */
