// Header-only C++ facade with the reference's class/method/member names on top of the C ABI
// (include/cuadmm_amd.h), so that callers written against the reference's SDPSolver
// (include/cuadmm/solver.h:30-248; src/main.cu:21-41) compile against this engine unchanged apart
// from the include line.  Differences: X/y/S are host copies fetched on demand (the reference exposes
// device pointers through DeviceDenseVector::vals), and failures throw std::runtime_error instead of
// printing and continuing (include/cuadmm/check.h:17-56).
#pragma once
#include <limits>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "cuadmm_amd.h"

namespace cuadmm_amd {

// Problem (include/cuadmm/problem.h:12-41; Problem::from_txt, src/problem.cu:11-83): the TXT directory of cuadmm_exe with the
// reference's member names -- blk_vals as (type, size) pairs, At in CSC over the constraints, sparse b and C; X / y / S stay
// empty (cold start: their data() is what main.cu hands to init).
class Problem {
 public:
  int vec_len = 0, con_num = 0, mat_num = 0, At_nnz = 0, b_nnz = 0, C_nnz = 0;
  std::vector<std::tuple<char, int>> blk_vals;
  std::vector<int> At_csc_col_ptrs, At_csc_row_ids, b_indices, C_indices;
  std::vector<double> At_csc_vals, b_vals, C_vals, X_vals, y_vals, S_vals;

  void from_txt(const std::string& prefix) {
    cuadmm_problem* p = nullptr;
    if (cuadmm_problem_from_txt(prefix.c_str(), &p) != CUADMM_OK) throw std::runtime_error(cuadmm_last_error());
    cuadmm_problem_view v;
    if (cuadmm_problem_view_get(p, &v) != CUADMM_OK) { cuadmm_problem_free(p); throw std::runtime_error(cuadmm_last_error()); }
    vec_len = v.vec_len; con_num = v.con_num; mat_num = v.mat_num; At_nnz = v.At_nnz; b_nnz = v.b_nnz; C_nnz = v.C_nnz;
    At_csc_col_ptrs.assign(v.At_csc_col_ptrs, v.At_csc_col_ptrs + v.con_num + 1);
    At_csc_row_ids.assign(v.At_csc_row_ids, v.At_csc_row_ids + v.At_nnz);
    At_csc_vals.assign(v.At_csc_vals, v.At_csc_vals + v.At_nnz);
    b_indices.assign(v.b_indices, v.b_indices + v.b_nnz); b_vals.assign(v.b_vals, v.b_vals + v.b_nnz);
    C_indices.assign(v.C_indices, v.C_indices + v.C_nnz); C_vals.assign(v.C_vals, v.C_vals + v.C_nnz);
    blk_vals.clear();
    for (int k = 0; k < v.mat_num; ++k) blk_vals.emplace_back(v.blk_vals[k] < 0 ? 'u' : 's', v.blk_vals[k] < 0 ? -v.blk_vals[k] : v.blk_vals[k]);
    cuadmm_problem_free(p);
  }
};

class SDPSolver {
 public:
  // results, named as in the reference (solver.h:149-161)
  int info_iter_num = 0;
  std::vector<double> info_pobj_arr, info_dobj_arr, info_errRp_arr, info_errRd_arr, info_relgap_arr, info_sig_arr,
      info_bscale_arr, info_Cscale_arr;
  double total_time = 0.0;
  int vec_len = 0, con_num = 0;

  struct HostVector {  // stands in for DeviceDenseVector<double>: .vals / .size, plus to_txt (memory.h:278-294)
    std::vector<double> data;
    double* vals = nullptr;
    int size = 0;
    void to_txt(const std::string& filename) const {
      if (cuadmm_write_dense_txt(filename.c_str(), data.data(), (int64_t)data.size()) != CUADMM_OK)
        throw std::runtime_error(cuadmm_last_error());
    }
  };
  HostVector X, y, S;

  SDPSolver() { check(cuadmm_create(&h_)); }
  ~SDPSolver() { cuadmm_destroy(h_); }
  SDPSolver(const SDPSolver&) = delete;
  SDPSolver& operator=(const SDPSolver&) = delete;

  void set_option(const char* key, double value) { check(cuadmm_set_option(h_, key, value)); }
  cuadmm_solver* handle() { return h_; }

  // SDPSolver::init, same argument list and defaults (solver.h:208-223)
  void init(int eig_stream_num_per_gpu, int cpu_eig_thread_num, int vec_len_, int con_num_, int* cpu_At_csc_col_ptrs,
            int* cpu_At_csc_row_ids, double* cpu_At_csc_vals, int At_nnz, int* cpu_b_indices, double* cpu_b_vals, int b_nnz,
            int* cpu_C_indices, double* cpu_C_vals, int C_nnz, int* cpu_blk_vals, int mat_num, double* cpu_X_vals = nullptr,
            double* cpu_y_vals = nullptr, double* cpu_S_vals = nullptr, double sig = 1.0) {
    check(cuadmm_init(h_, eig_stream_num_per_gpu, cpu_eig_thread_num, vec_len_, con_num_, cpu_At_csc_col_ptrs,
                      cpu_At_csc_row_ids, cpu_At_csc_vals, At_nnz, cpu_b_indices, cpu_b_vals, b_nnz, cpu_C_indices, cpu_C_vals,
                      C_nnz, cpu_blk_vals, mat_num, cpu_X_vals, cpu_y_vals, cpu_S_vals, sig));
    vec_len = vec_len_;
    con_num = con_num_;
  }

  // SDPDuoSolver::init (duo_solver.h:236-255): two leading arguments more, default sig = 2e2
  void duo_init(bool if_gpu_eig_mom, int device_num_requested, int eig_stream_num_per_gpu, int cpu_eig_thread_num, int vec_len_,
                int con_num_, int* cpu_At_csc_col_ptrs, int* cpu_At_csc_row_ids, double* cpu_At_csc_vals, int At_nnz,
                int* cpu_b_indices, double* cpu_b_vals, int b_nnz, int* cpu_C_indices, double* cpu_C_vals, int C_nnz,
                int* cpu_blk_vals, int mat_num, double* cpu_X_vals = nullptr, double* cpu_y_vals = nullptr,
                double* cpu_S_vals = nullptr, double sig = 2e2) {
    check(cuadmm_duo_init(h_, if_gpu_eig_mom ? 1 : 0, device_num_requested, eig_stream_num_per_gpu, cpu_eig_thread_num, vec_len_,
                          con_num_, cpu_At_csc_col_ptrs, cpu_At_csc_row_ids, cpu_At_csc_vals, At_nnz, cpu_b_indices, cpu_b_vals,
                          b_nnz, cpu_C_indices, cpu_C_vals, C_nnz, cpu_blk_vals, mat_num, cpu_X_vals, cpu_y_vals, cpu_S_vals, sig));
    vec_len = vec_len_;
    con_num = con_num_;
  }

  // option "accel" (set_option before init): [memory, taken, accepted, rejected, restarts, columns, ms, ring bytes]; not in the reference
  struct AccelInfo { int memory; long long taken, accepted, rejected, restarts; int columns; double ms, ring_bytes; };
  AccelInfo accel_info() const {
    double o[8] = {0};
    check(cuadmm_get_accel_info(h_, o));
    return AccelInfo{(int)o[0], (long long)o[1], (long long)o[2], (long long)o[3], (long long)o[4], (int)o[5], o[6], o[7]};
  }

  // how the last solve ended (cuadmm_get_status); option "infeas_check" adds the two infeasible statuses; not in the reference
  enum Status { kNoSolve = 0, kConverged = 1, kIterationLimit = 2, kPrimalInfeasible = 3, kDualInfeasible = 4, kCertifiedGap = 5 };
  struct StatusInfo { Status status; int iteration; long long checks; double scalar, eta, radius, ms, bytes; };
  StatusInfo status() const {
    double o[8] = {0};
    check(cuadmm_get_status(h_, o));
    return StatusInfo{(Status)(int)o[0], (int)o[1], (long long)o[2], o[3], o[4], o[5], o[6], o[7]};
  }
  // the ray behind kPrimalInfeasible (y, con_num entries, b'y = 1) or kDualInfeasible (X, vec_len entries, <C, X> = -1); throws otherwise
  std::vector<double> certificate() {
    const StatusInfo st = status();
    int vl = 0, cn = 0, mn = 0;
    check(cuadmm_get_dims(h_, &vl, &cn, &mn));
    std::vector<double> ray((size_t)(st.status == kDualInfeasible ? vl : cn));
    check(cuadmm_get_certificate(h_, st.status == kDualInfeasible ? nullptr : ray.data(), st.status == kDualInfeasible ? ray.data() : nullptr));
    return ray;
  }

  // trace bounds (one per block; PSD: tr X_k <= R_k, unconstrained: ||x_k|| <= R_k) for lower_bound() and option "gap_check";
  // an empty vector clears them; not in the reference
  void set_trace_bounds(const std::vector<double>& R) { check(cuadmm_set_trace_bounds(h_, R.empty() ? nullptr : R.data(), (int)R.size())); }
  // cuadmm_lower_bound at the current y; per_block (may be null): resized to 2 mat_num, [2k] nu_k, [2k + 1] ||S^_k||_F
  struct LowerBound { double lower_bound, bty, penalty, gap; int worst_block; double worst_term, ms, bytes; };
  LowerBound lower_bound(std::vector<double>* per_block = nullptr) {
    double o[8] = {0};
    if (per_block) {
      int vl = 0, cn = 0, mn = 0;
      check(cuadmm_get_dims(h_, &vl, &cn, &mn));
      per_block->assign(2 * (size_t)mn, 0.0);
    }
    check(cuadmm_lower_bound(h_, o, per_block ? per_block->data() : nullptr));
    return LowerBound{o[0], o[1], o[2], o[3], (int)o[4], o[5], o[6], o[7]};
  }
  // option "gap_check" in the last solve (cuadmm_get_gap_info)
  struct GapInfo { long long checks; double best_lower_bound; int best_iteration; double last_lower_bound, last_gap, ms, bytes; int verdict_iteration; };
  GapInfo gap_info() const {
    double o[8] = {0};
    check(cuadmm_get_gap_info(h_, o));
    return GapInfo{(long long)o[0], o[1], (int)o[2], o[3], o[4], o[5], o[6], (int)o[7]};
  }

  // cuadmm_evaluate: KKT and DIMACS report of a point (host pointers in the caller's units, null: the current vector); per_block (may be
  // null): resized to 6 mat_num, [6k ..] = ||X_k||, vX_k, ||S_k||, vS_k, <X_k, S_k>, ||Rd_k||; not in the reference
  struct Evaluation { double pobj, dobj, norm_Rp, norm_Rd, vX, vS, XS, norm_b, norm_C, err[6], ms; };
  Evaluation evaluate(const double* X = nullptr, const double* y = nullptr, const double* S = nullptr, std::vector<double>* per_block = nullptr) {
    double o[16] = {0};
    if (per_block) {
      int vl = 0, cn = 0, mn = 0;
      check(cuadmm_get_dims(h_, &vl, &cn, &mn));
      per_block->assign(6 * (size_t)mn, 0.0);
    }
    check(cuadmm_evaluate(h_, X, y, S, o, per_block ? per_block->data() : nullptr));
    return Evaluation{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], {o[9], o[10], o[11], o[12], o[13], o[14]}, o[15]};
  }

  // cuadmm_lambda_min: certified lower bounds on lambda_min of the blocks of X (which = 0), S (1) or C - A'y (2); per_block (may be
  // null): resized to 3 mat_num, [3k ..] = lo_k (certified), hi_k (an estimate), flag; not in the reference
  struct LambdaMin { double lambda_min; int block; double dimacs, lower_bound; int unrefined, psd_at_floor; double ms, bytes; };
  LambdaMin lambda_min(int which, int steps = 12, std::vector<double>* per_block = nullptr) {
    double o[8] = {0};
    if (per_block) {
      int vl = 0, cn = 0, mn = 0;
      check(cuadmm_get_dims(h_, &vl, &cn, &mn));
      per_block->assign(3 * (size_t)mn, 0.0);
    }
    check(cuadmm_lambda_min(h_, which, steps, o, per_block ? per_block->data() : nullptr));
    return LambdaMin{o[0], (int)o[1], o[2], o[3], (int)o[4], (int)o[5], o[6], o[7]};
  }

  // cuadmm_lowrank: numerical rank and a factor M_k ~ L_k L_k' of the blocks of X (which = 0) or S (1) by pivoted Cholesky; per_block:
  // [6k ..] = rank, resid, dneg, trace, flag, offset of L_k in L; L: n_k min(n_k, rmax) doubles per PSD block, column by column; piv: as
  // many ints, a block's pivots at the same offset, -1 elsewhere; not in the reference
  struct LowRank {
    double rank_sum; int rank_max, block; double resid, dneg; int capped; double ms, bytes;
    std::vector<double> per_block, L;
    std::vector<int> piv;
  };
  LowRank lowrank(int which, double tol, int rmax, bool factors = true) {
    double o[8] = {0};
    int vl = 0, cn = 0, mn = 0;
    long long count = 0;
    check(cuadmm_get_dims(h_, &vl, &cn, &mn));
    check(cuadmm_lowrank_size(h_, rmax, &count));
    LowRank r;
    r.per_block.assign(6 * (size_t)mn, 0.0);
    if (factors) { r.L.assign((size_t)count, 0.0); r.piv.assign((size_t)count, -1); }
    check(cuadmm_lowrank(h_, which, tol, rmax, o, r.per_block.data(), factors ? r.L.data() : nullptr, factors ? r.piv.data() : nullptr));
    r.rank_sum = o[0]; r.rank_max = (int)o[1]; r.block = (int)o[2]; r.resid = o[3]; r.dneg = o[4]; r.capped = (int)o[5]; r.ms = o[6]; r.bytes = o[7];
    return r;
  }

  // cuadmm_set_lowrank: X (which = 0) or S (1) <- L_k L_k' per PSD block between two solves; L in the layout of LowRank::L for this rmax,
  // ranks: mat_num column counts (per_block[6k] of a LowRank; unconstrained blocks ignored); not in the reference
  struct LowRankStart { int blocks; double rank_sum, ms, bytes_staged; };
  LowRankStart set_lowrank(int which, const double* L, const int* ranks, int rmax, double sig = 0.0) {
    double o[4] = {0};
    check(cuadmm_set_lowrank(h_, which, L, ranks, rmax, sig, o));
    return LowRankStart{(int)o[0], o[1], o[2], o[3]};
  }

  // cuadmm_block_multiply: W_k = M_k V_k per PSD block, M = X (which = 0), S (1) or C - A'y (2); V in the layout of LowRank::L for this rmax,
  // ranks: mat_num column counts; W in the same layout, per_block: [4k ..] = ||W_k||_F, <V_k, W_k>, ||V_k||_F, flag; not in the reference
  struct BlockMultiply {
    double norm, inner; int block; double block_norm; int blocks; double rank_sum, ms, bytes;
    std::vector<double> W, per_block;
  };
  BlockMultiply block_multiply(int which, const double* V, const int* ranks, int rmax) {
    double o[8] = {0};
    int vl = 0, cn = 0, mn = 0;
    long long count = 0;
    check(cuadmm_get_dims(h_, &vl, &cn, &mn));
    check(cuadmm_lowrank_size(h_, rmax, &count));
    BlockMultiply r;
    r.W.assign((size_t)count + 1, 0.0);
    r.per_block.assign(4 * (size_t)mn, 0.0);
    check(cuadmm_block_multiply(h_, which, V, ranks, rmax, r.W.data(), o, r.per_block.data()));
    r.W.resize((size_t)count);
    r.norm = o[0]; r.inner = o[1]; r.block = (int)o[2]; r.block_norm = o[3]; r.blocks = (int)o[4]; r.rank_sum = o[5]; r.ms = o[6]; r.bytes = o[7];
    return r;
  }

  // cuadmm_lowrank_grad: f = <C, x> - y'r + (sigma / 2) ||r||^2 and G_k = 2 (C - A'(y - sigma r))_k L_k at the factors L (x: X with every
  // PSD block replaced by L_k L_k', r = A x - b); L, ranks, rmax as block_multiply's V; y: con_num values or null for the resident y; G in
  // the layout of L, per_block: [4k ..] = <C_k, x_k>, ||G_k||_F, <L_k, G_k>, ||L_k||_F^2; Shat only with want_S; not in the reference
  struct LowRankGrad {
    double f, cx, yr, rnorm, gnorm, lg, ms, bytes;
    std::vector<double> G, r, Shat, per_block;
  };
  LowRankGrad lowrank_grad(const double* L, const int* ranks, int rmax, const double* y = nullptr, double sigma = 0.0, bool want_S = false) {
    double o[8] = {0};
    int vl = 0, cn = 0, mn = 0;
    long long count = 0;
    check(cuadmm_get_dims(h_, &vl, &cn, &mn));
    check(cuadmm_lowrank_size(h_, rmax, &count));
    LowRankGrad g;
    g.G.assign((size_t)count + 1, 0.0);
    g.r.assign((size_t)cn + 1, 0.0);
    if (want_S) g.Shat.assign((size_t)vl + 1, 0.0);
    g.per_block.assign(4 * (size_t)mn, 0.0);
    check(cuadmm_lowrank_grad(h_, L, ranks, rmax, y, sigma, g.G.data(), g.r.data(), want_S ? g.Shat.data() : nullptr, o, g.per_block.data()));
    g.G.resize((size_t)count);
    g.r.resize((size_t)cn);
    if (want_S) g.Shat.resize((size_t)vl);
    g.f = o[0]; g.cx = o[1]; g.yr = o[2]; g.rnorm = o[3]; g.gnorm = o[4]; g.lg = o[5]; g.ms = o[6]; g.bytes = o[7];
    return g;
  }

  // cuadmm_lowrank_line: the quartic t -> f(L + t D) of lowrank_grad's f (coef: c0 .. c4) and its global minimiser on [0, t_max]
  // (t_max <= 0: coefficients only); L, D, ranks, rmax as lowrank_grad's L; r(t) = r + t p + t^2 q; per_block: [4k ..] = <C_k, x0_k>,
  // <C_k, x1_k>, <C_k, x2_k>, flag; not in the reference
  struct LowRankLine {
    double coef[5], t, f, decrease, pnorm, qnorm, ms, bytes;
    int critical;
    std::vector<double> r, p, q, per_block;
  };
  LowRankLine lowrank_line(const double* L, const double* D, const int* ranks, int rmax, const double* y = nullptr, double sigma = 0.0,
                           double t_max = std::numeric_limits<double>::infinity()) {
    double o[8] = {0};
    int vl = 0, cn = 0, mn = 0;
    check(cuadmm_get_dims(h_, &vl, &cn, &mn));
    LowRankLine g;
    g.r.assign((size_t)cn + 1, 0.0);
    g.p.assign((size_t)cn + 1, 0.0);
    g.q.assign((size_t)cn + 1, 0.0);
    g.per_block.assign(4 * (size_t)mn, 0.0);
    check(cuadmm_lowrank_line(h_, L, D, ranks, rmax, y, sigma, t_max, g.coef, g.r.data(), g.p.data(), g.q.data(), o, g.per_block.data()));
    g.r.resize((size_t)cn);
    g.p.resize((size_t)cn);
    g.q.resize((size_t)cn);
    g.t = o[0]; g.f = o[1]; g.decrease = o[2]; g.pnorm = o[3]; g.qnorm = o[4]; g.critical = (int)o[5]; g.ms = o[6]; g.bytes = o[7];
    return g;
  }

  // cuadmm_lowrank_refine: `steps` steps of Polak-Ribiere+ conjugate gradients on lowrank_grad's f with lowrank_line's line search, the
  // factors resident on the device; L, ranks, rmax, y, sigma as lowrank_grad's; trace: 16 doubles per step begun ([gg, go, gd, beta,
  // slope, restart, c0 .. c4, t, f(t), ms, 0, 0]); reason: 0 all steps, 1 t = 0, 2 gtol, 3 not finite, 4 unbounded quartic; not in the
  // reference
  struct LowRankRefine {
    std::vector<double> L, trace, r;
    int steps, reason;
    double f0, f, gnorm, ms, bytes;
  };
  LowRankRefine lowrank_refine(const double* L, const int* ranks, int rmax, const double* y = nullptr, double sigma = 1.0, int steps = 10,
                               double t_max = std::numeric_limits<double>::infinity(), double gtol = 0.0) {
    double o[8] = {0};
    int vl = 0, cn = 0, mn = 0;
    long long count = 0;
    check(cuadmm_get_dims(h_, &vl, &cn, &mn));
    check(cuadmm_lowrank_size(h_, rmax, &count));
    LowRankRefine g;
    g.L.assign((size_t)count + 1, 0.0);
    g.trace.assign(16 * (size_t)(steps > 0 ? steps : 0) + 1, 0.0);
    g.r.assign((size_t)cn + 1, 0.0);
    check(cuadmm_lowrank_refine(h_, L, ranks, rmax, y, sigma, steps, t_max, gtol, g.L.data(), g.trace.data(), o, g.r.data()));
    g.steps = (int)o[0]; g.reason = (int)o[1]; g.f0 = o[2]; g.f = o[3]; g.gnorm = o[4]; g.ms = o[5]; g.bytes = o[6];
    g.L.resize((size_t)count);
    g.trace.resize(16 * (size_t)(g.steps + (g.reason ? 1 : 0)));
    g.r.resize((size_t)cn);
    return g;
  }

  // cuadmm_update_bC: new b and / or C on the factored solver (nnz < 0: unchanged); not in the reference
  void update_bC(const int* cpu_b_indices, const double* cpu_b_vals, int b_nnz, const int* cpu_C_indices, const double* cpu_C_vals,
                 int C_nnz, bool keep_iterate = true, double sig = 0.0) {
    check(cuadmm_update_bC(h_, cpu_b_indices, cpu_b_vals, b_nnz, cpu_C_indices, cpu_C_vals, C_nnz, keep_iterate ? 1 : 0, sig));
  }

  // cuadmm_update_A: new values of A on the pattern of init (the caller's order at init); not in the reference
  void update_A(const double* cpu_At_csc_vals, int At_nnz, bool keep_iterate = true, double sig = 0.0) {
    check(cuadmm_update_A(h_, cpu_At_csc_vals, At_nnz, keep_iterate ? 1 : 0, sig));
  }
  struct UpdateInfo { long long updates; double wall_ms, host_factor_ms, device_solve_ms; long long orderings; double bytes_to_device; };
  UpdateInfo update_info() const {
    double o[6] = {0};
    check(cuadmm_get_update_info(h_, o));
    return UpdateInfo{(long long)o[0], o[1], o[2], o[3], (long long)o[4], o[5]};
  }

  // SDPSolver::solve, same argument list and defaults (solver.h:236-244)
  void solve(int max_iter, double stop_tol, int sig_update_threshold = 500, int sig_update_stage_1 = 50,
             int sig_update_stage_2 = 100, int switch_admm = (int)1.1e4, double sigscale = 1.05, bool if_first = true) {
    int rc = cuadmm_solve(h_, max_iter, stop_tol, sig_update_threshold, sig_update_stage_1, sig_update_stage_2, switch_admm,
                          sigscale, if_first ? 1 : 0);
    fetch();
    check(rc);
  }

 private:
  cuadmm_solver* h_ = nullptr;
  static void check(int rc) {
    if (rc < 0) throw std::runtime_error(cuadmm_last_error());
  }
  void fetch_vec(HostVector& v, int n, int (*get)(cuadmm_solver*, double*)) {
    v.data.resize((size_t)n);
    check(get(h_, v.data.data()));
    v.vals = v.data.data();
    v.size = n;
  }
  void fetch() {
    int64_t b = 0, e = 0;
    check(cuadmm_get_shard(h_, &b, &e, nullptr, nullptr));
    fetch_vec(X, (int)(e - b), cuadmm_get_X);
    fetch_vec(S, (int)(e - b), cuadmm_get_S);
    fetch_vec(y, con_num, cuadmm_get_y);
    info_iter_num = cuadmm_get_info_iter_num(h_);
    std::vector<double>* arrs[8] = {&info_pobj_arr, &info_dobj_arr, &info_errRp_arr, &info_errRd_arr,
                                    &info_relgap_arr, &info_sig_arr, &info_bscale_arr, &info_Cscale_arr};
    for (int k = 0; k < 8; ++k) {
      std::vector<double> tmp(1 << 20);
      int n = cuadmm_get_info_array(h_, k, tmp.data(), (int)tmp.size());
      if (n < 0) n = 0;
      arrs[k]->assign(tmp.begin(), tmp.begin() + n);
    }
    total_time = cuadmm_get_total_time(h_);
  }
};

}  // namespace cuadmm_amd
