// cuadmm_exe <dir/> : the reference's command line front end (src/main.cu:8-44) on top of the C ABI.
//
// Same positional form, same constants: eig_streams=15, cpu_eig_threads=30, sig=1.0 and
// solve(1e6, 1e-3, /*sig_update_threshold=*/false -> 0, 50, 100, 5000) (main.cu:10-11,23,39), reads
// <dir/>{blk,con_num,At,b,C}.txt and writes <dir/>X_opt.txt with "%.32f" per line (memory.h:278-294).
// Optional trailing --key=value arguments (not in the reference) override the solve parameters:
//   --max_iter= --stop_tol= --threshold= --stage1= --stage2= --switch_admm= --sigscale= --sig= --device= --quiet
//   --accel=M: safeguarded Anderson acceleration with memory M (option "accel"); prints "accel: taken a, accepted b, rejected c,
//   restarts d" after the solve and adds the four numbers to the sidecar
//   --infeas=P --infeas_tol=T: infeasibility check every P iterations (options "infeas_check", "infeas_tol"); a certificate ends that solve
//   with "Solver ended: primal infeasible ..." in the summary, and a --then sequence goes on with its next stage.  The sidecar carries
//   "status" ("converged", "iteration_limit", "primal_infeasible", "dual_infeasible") with or without the check
//   --trace-bounds=FILE|auto: one number R_k per line of blk.txt (PSD block: tr X_k <= R_k, unconstrained: ||x_k|| <= R_k), or "auto":
//   read off the constraints (cuadmm_trace_bounds_detect; an error when a block has none).  With them the sidecar carries "lower_bound"
//   (cuadmm_lower_bound at the returned y) and "certified_gap"; without the flag it is what it was
//   --gap=P --gap_tol=T: certified-gap check every P iterations (options "gap_check", "gap_tol"; needs --trace-bounds); status "certified_gap"
//   --kkt: the KKT and DIMACS report of the returned point behind every solve (cuadmm_evaluate at the current X, y, S), printed and added to
//   the sidecar as "kkt"
//   --kkt-point=<dir2/>: no solve; the report of the point in <dir2/>{X,y,S}.txt (one number per line, as this program writes X_opt.txt; a
//   missing file: that vector is zero) is printed and, with --json, written as the sidecar's "kkt"
//   --lambda-min[=T]: behind every solve, certified lower bounds on lambda_min of the blocks of X, S and C - A'y (cuadmm_lambda_min with T
//   bisection steps, default 12), one line each, and "lambda_min" in the sidecar
//   --lowrank=TOL[,RMAX]: behind every solve, the numerical rank of every block of X and of S by pivoted Cholesky (cuadmm_lowrank with the
//   relative tolerance TOL and at most RMAX columns per block, default the largest block size), one line each, and "lowrank" in the sidecar
//   --lowrank-out=DIR/ (with --lowrank): the factors, DIR/L_X_<k>.txt and DIR/L_S_<k>.txt per PSD block k, n_k r_k numbers column by column
//   --start-lowrank=DIR/: the first solve starts from factors as --lowrank-out writes them (cuadmm_set_lowrank): DIR/L_X_<k>.txt and
//   DIR/L_S_<k>.txt hold n_k r_k numbers, so r_k = count / n_k; a matrix none of whose files is present is left alone, otherwise a missing
//   block has rank 0; DIR/y.txt (con_num numbers), where present, is y.  A file whose count is no multiple of n_k or exceeds n_k^2 ends the
//   program with exit code 1 before any device work.  One line per matrix set, and "start_lowrank" in the sidecar
//   --block-mult=X|S|dual,DIR/ (repeatable): behind every solve, W_k = M_k V_k for every PSD block of X, S or C - A'y (cuadmm_block_multiply)
//   with V_k from factor files as --lowrank-out writes them, read by the reader of --start-lowrank: DIR/L_X_<k>.txt where any is present,
//   otherwise DIR/L_S_<k>.txt (files of the matrix that is not used are not opened); a missing block has rank 0.  One line per call, and "block_mult" (one object per call) in the sidecar
//   --lowrank-grad=DIR/[,SIGMA]: behind every solve, value and gradient of <C, x> - y'r + (SIGMA / 2) ||r||^2 at the factors DIR/L_X_<k>.txt
//   (as --lowrank-out writes them; else DIR/L_S_<k>.txt) with y from DIR/y.txt when present, else the resident y (cuadmm_lowrank_grad);
//   one line, and "lowrank_grad" in the sidecar.  --lowrank-grad-out=DIR2/: DIR2/G_<k>.txt per PSD block (as W_<k>.txt) and DIR2/r.txt
//   --lowrank-line=LDIR/,DDIR/[,SIGMA[,TMAX]]: behind every solve, the quartic t -> f(L + t D) of that value along the direction read from
//   DDIR/ (factor files as LDIR/'s, the same ranks), y from LDIR/y.txt when present, and its minimiser on [0, TMAX] (default: inf, which
//   needs SIGMA > 0) (cuadmm_lowrank_line); one line with c0 .. c4, t* and f(t*), and "lowrank_line" in the sidecar
//   --lowrank-refine=DIR/[,SIGMA[,STEPS[,TMAX]]]: behind every solve, STEPS (10) steps of conjugate gradients on that value over the factors
//   read from DIR/ (as --lowrank-out writes them) with y from DIR/y.txt when present, SIGMA (1) >= 0, TMAX (inf) > 0
//   (cuadmm_lowrank_refine); one line per step and "lowrank_refine" in the sidecar
//   --lowrank-refine-out=DIR2/ (with --lowrank-refine): the refined factors, DIR2/L_X_<k>.txt as --start-lowrank reads them
//   --block-mult-out=DIR2/ (with --block-mult): DIR2/W_<k>.txt per PSD block k, n_k r_k numbers column by column with 17 significant
//   digits (of the last --block-mult where there are several)
//   --json=<file>: a sidecar with the run's figures (iterations, residuals, iters/s, per-phase milliseconds, the projection's
//   nominal TFLOP/s = 10.67 sum n^3 per projection and the vector kernels' algorithmic GB/s: SURVEY.md 8d); switches the
//   engine's per-phase HIP-event timers on (option "profile").  Nothing is written unless asked for: the reference writes X_opt.txt only.
//   --then=<dir2/> (repeatable): after the solve, read ONLY b.txt and C.txt from <dir2/> (either may be absent: unchanged), replace
//   them on the factored solver (cuadmm_update_bC, warm start), solve with the same parameters and write <dir2/>X_opt.txt; one
//   sidecar per stage: <file>, <file>.1, ...  A receding-horizon sequence pays for the ordering and the factor once.
//   --then-A=<dir2/> (repeatable, in order with --then=): <dir2/> holds a whole problem on the SAME sparsity pattern of A (blk, con_num
//   and the index columns of At.txt identical, checked before anything changes); its values of A replace the solver's
//   (cuadmm_update_A: refactorisation on the analysis of the first init, warm start), then its b and C as with --then=, solve, write
//   <dir2/>X_opt.txt.
#include <dirent.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "cuadmm_amd.h"

static bool opt(const char* arg, const char* key, double& out) {
  size_t n = strlen(key);
  if (strncmp(arg, key, n) == 0 && arg[n] == '=') { out = atof(arg + n + 1); return true; }
  return false;
}

static const char* const kkt_names[16] = {"pobj", "dobj", "norm_Rp", "norm_Rd", "vX", "vS", "XS", "norm_b", "norm_C", "err1", "err2", "err3", "err4", "err5", "err6", "ms"};
// "kkt": {...} with the sixteen numbers of cuadmm_evaluate and "per_block": mat_num rows of six
static void write_kkt(FILE* f, const double* k, const std::vector<double>& pb) {
  fprintf(f, " \"kkt\": {");
  for (int q = 0; q < 16; ++q) fprintf(f, "\"%s\": %.17g, ", kkt_names[q], k[q]);
  fprintf(f, "\"per_block\": [");
  for (size_t b = 0; b < pb.size() / 6; ++b)
    fprintf(f, "%s[%.17g, %.17g, %.17g, %.17g, %.17g, %.17g]", b ? ", " : "", pb[6 * b], pb[6 * b + 1], pb[6 * b + 2], pb[6 * b + 3], pb[6 * b + 4], pb[6 * b + 5]);
  fprintf(f, "]}");
}
static void print_kkt(const double* k, const std::vector<double>& pb) {
  printf("\n KKT report (cuadmm_evaluate):\n");
  printf("  pobj = %.10e, dobj = %.10e, <X,S> = %.3e\n", k[0], k[1], k[6]);
  printf("  ||AX - b|| = %.3e, ||A'y + S - C|| = %.3e, ||P+(-X)|| = %.3e, ||P+(-S)|| = %.3e (||b|| = %.3e, ||C|| = %.3e)\n", k[2], k[3], k[4], k[5], k[7], k[8]);
  printf("  DIMACS: err1 = %.3e, err2 = %.3e, err3 = %.3e, err4 = %.3e, err5 = %.3e, err6 = %.3e (err2, err4: Frobenius norm of the negative parts)\n",
         k[9], k[10], k[11], k[12], k[13], k[14]);
  size_t wx = 0, ws = 0, wr = 0;
  for (size_t b = 0; b < pb.size() / 6; ++b) {
    if (pb[6 * b + 1] > pb[6 * wx + 1]) wx = b;
    if (pb[6 * b + 3] > pb[6 * ws + 3]) ws = b;
    if (pb[6 * b + 5] > pb[6 * wr + 5]) wr = b;
  }
  if (!pb.empty())
    printf("  worst blocks: vX %.3e (block %zu), vS %.3e (block %zu), ||Rd_k|| %.3e (block %zu); %.3f ms\n", pb[6 * wx + 1], wx, pb[6 * ws + 3], ws, pb[6 * wr + 5], wr, k[15]);
}
static const char* const lm_names[3] = {"X", "S", "dual"};
// "lambda_min": {"steps": T, "X": {...}, "S": {...}, "dual": {...}} with the eight numbers of cuadmm_lambda_min each (NaN: null)
static void write_lambda_min(FILE* f, int steps, const double (*lm)[8]) {
  fprintf(f, " \"lambda_min\": {\"steps\": %d", steps);
  for (int w = 0; w < 3; ++w) {
    const double* o = lm[w];
    fprintf(f, ", \"%s\": {\"lambda_min\": %.17g, \"block\": %.0f, \"dimacs\": %.17g, \"lower_bound\": ", lm_names[w], o[0], o[1], o[2]);
    if (std::isfinite(o[3])) fprintf(f, "%.17g", o[3]); else fprintf(f, "null");
    fprintf(f, ", \"unrefined\": %.0f, \"psd_at_floor\": %.0f, \"ms\": %.17g, \"bytes\": %.0f}", o[4], o[5], o[6], o[7]);
  }
  fprintf(f, "}");
}
// --lowrank: what cuadmm_lowrank returned for X (0) and S (1)
struct LowRankReport {
  double tol = 0;
  int rmax = 0;
  double o[2][8] = {{0}};
  std::vector<double> pb[2], L[2];
};
// "lowrank": {"tol": .., "rmax": .., "X": {...}, "S": {...}} with the eight numbers of cuadmm_lowrank each and "rank", "flag" per block
static void write_lowrank(FILE* f, const LowRankReport& r) {
  fprintf(f, " \"lowrank\": {\"tol\": %.17g, \"rmax\": %d", r.tol, r.rmax);
  for (int w = 0; w < 2; ++w) {
    const double* o = r.o[w];
    fprintf(f, ", \"%s\": {\"rank_sum\": %.0f, \"rank_max\": %.0f, \"block\": %.0f, \"resid_sum\": ", lm_names[w], o[0], o[1], o[2]);
    if (std::isfinite(o[3])) fprintf(f, "%.17g", o[3]); else fprintf(f, "null");
    fprintf(f, ", \"dneg_min\": %.17g, \"capped\": %.0f, \"ms\": %.17g, \"bytes\": %.0f, \"rank\": [", o[4], o[5], o[6], o[7]);
    for (size_t b = 0; b < r.pb[w].size() / 6; ++b) fprintf(f, "%s%.0f", b ? ", " : "", r.pb[w][6 * b]);
    fprintf(f, "], \"flag\": [");
    for (size_t b = 0; b < r.pb[w].size() / 6; ++b) fprintf(f, "%s%.0f", b ? ", " : "", r.pb[w][6 * b + 4]);
    fprintf(f, "]}");
  }
  fprintf(f, "}");
}
// --start-lowrank: the factors of X (0) and S (1) in the layout of cuadmm_set_lowrank, and what the calls returned
struct LowRankStart {
  bool have[2] = {false, false}, have_y = false;
  int rmax[2] = {1, 1};
  std::vector<int> ranks[2];
  std::vector<double> L[2], y;
  double o[2][4] = {{0}};
};
// DIR/L_<X|S>_<k>.txt of every PSD block -> st (only >= 0: that matrix alone, the other's files are not opened); false (with a message) on
// a file whose count does not fit its block
static bool read_lowrank_start(const std::string& dir, const cuadmm_problem_view& v, LowRankStart& st, int only = -1) {
  for (int w = 0; w < 2; ++w) {
    if (only >= 0 && w != only) continue;
    std::vector<std::vector<double>> cols((size_t)v.mat_num);
    st.ranks[w].assign((size_t)v.mat_num, 0);
    for (int k = 0; k < v.mat_num; ++k) {
      const long long n = v.blk_vals[k];
      if (n <= 0) continue;
      const std::string fn = dir + "L_" + (w == 0 ? "X" : "S") + "_" + std::to_string(k) + ".txt";
      FILE* f = fopen(fn.c_str(), "r");
      if (!f) continue;
      st.have[w] = true;
      double x = 0;
      while ((long long)cols[k].size() <= n * n && fscanf(f, "%lf", &x) == 1) cols[k].push_back(x);
      fclose(f);
      const long long count = (long long)cols[k].size();
      if (count % n != 0 || count > n * n) {
        std::cerr << "--start-lowrank: '" << fn << "' holds " << (count > n * n ? "more than " : "") << std::min(count, n * n) << " numbers; block " << k
                  << " of size " << n << " takes a multiple of " << n << ", at most " << n * n << std::endl;
        return false;
      }
      st.ranks[w][k] = (int)(count / n);
      st.rmax[w] = std::max(st.rmax[w], st.ranks[w][k]);
    }
    if (!st.have[w]) continue;
    st.L[w].clear();
    for (int k = 0; k < v.mat_num; ++k) {
      const long long n = v.blk_vals[k];
      if (n <= 0) continue;
      const size_t at = st.L[w].size();
      st.L[w].resize(at + (size_t)(n * std::min<long long>(n, st.rmax[w])), 0.0);
      std::copy(cols[k].begin(), cols[k].end(), st.L[w].begin() + at);
    }
    st.L[w].push_back(0.0);      // never empty
  }
  return true;
}
// "start_lowrank": {"X": {...}, "S": {...}} with the four numbers of cuadmm_set_lowrank for each matrix that was set
static void write_start(FILE* f, const LowRankStart& st) {
  fprintf(f, " \"start_lowrank\": {\"y\": %s", st.have_y ? "true" : "false");
  for (int w = 0; w < 2; ++w)
    if (st.have[w])
      fprintf(f, ", \"%s\": {\"blocks\": %.0f, \"rank_sum\": %.0f, \"ms\": %.17g, \"bytes_staged\": %.0f, \"rmax\": %d}", w == 0 ? "X" : "S", st.o[w][0], st.o[w][1],
              st.o[w][2], st.o[w][3], st.rmax[w]);
  fprintf(f, "}");
}
// --block-mult: one call of cuadmm_block_multiply -- the matrix, the factors (those of X where DIR/ has any, else those of S) and the results
struct BlockMultCall {
  int which = 0, rmax = 1;
  std::string dir;
  std::vector<int> ranks;
  std::vector<double> V, W;
  double o[8] = {0};
};
static bool read_block_mult(const cuadmm_problem_view& v, BlockMultCall& c) {
  LowRankStart st;
  if (!read_lowrank_start(c.dir, v, st, 0)) return false;                 // the factors of X; those of S only where there are none
  if (!st.have[0] && !read_lowrank_start(c.dir, v, st, 1)) return false;
  const int w = st.have[0] ? 0 : 1;
  if (!st.have[w]) { std::cerr << "--block-mult: no factor file L_X_<k>.txt or L_S_<k>.txt in '" << c.dir << "'" << std::endl; return false; }
  c.rmax = st.rmax[w]; c.ranks = st.ranks[w]; c.V = st.L[w];
  c.W.assign(c.V.size(), 0.0);
  return true;
}
// "block_mult": [{...}, ...] with the eight numbers of cuadmm_block_multiply per call
static void write_block_mult(FILE* f, const std::vector<BlockMultCall>& calls) {
  fprintf(f, " \"block_mult\": [");
  for (size_t q = 0; q < calls.size(); ++q) {
    const double* o = calls[q].o;
    fprintf(f, "%s{\"which\": \"%s\", \"rmax\": %d, \"norm\": %.17g, \"inner\": %.17g, \"block\": %.0f, \"block_norm\": %.17g, \"blocks\": %.0f, \"rank_sum\": %.0f, "
            "\"ms\": %.17g, \"bytes\": %.0f}", q ? ", " : "", lm_names[calls[q].which], calls[q].rmax, o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]);
  }
  fprintf(f, "]");
}
// --lowrank-grad: the factors, y (when DIR/y.txt exists), sigma and the results of cuadmm_lowrank_grad
struct LowRankGradCall {
  bool on = false, have_y = false;
  int rmax = 1;
  double sigma = 0;
  std::string dir;
  std::vector<int> ranks;
  std::vector<double> L, G, y, r;
  double o[8] = {0};
};
// "lowrank_grad": {...} with the eight numbers of cuadmm_lowrank_grad
static void write_lowrank_grad(FILE* f, const LowRankGradCall& c) {
  const double* o = c.o;
  fprintf(f, " \"lowrank_grad\": {\"sigma\": %.17g, \"rmax\": %d, \"y\": %s, \"f\": %.17g, \"cx\": %.17g, \"yr\": %.17g, \"rnorm\": %.17g, \"gnorm\": %.17g, "
          "\"lg\": %.17g, \"ms\": %.17g, \"bytes\": %.0f}", c.sigma, c.rmax, c.have_y ? "true" : "false", o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]);
}
// --lowrank-line: the factors, the direction, y (when LDIR/y.txt exists), sigma, t_max and the results of cuadmm_lowrank_line
struct LowRankLineCall {
  bool on = false, have_y = false;
  int rmax = 1;
  double sigma = 0, t_max = INFINITY;
  std::string ldir, ddir;
  std::vector<int> ranks;
  std::vector<double> L, D, y;
  double coef[5] = {0}, o[8] = {0};
};
// "lowrank_line": {...} with the coefficients and the eight numbers of cuadmm_lowrank_line (t_max: null for inf)
static void write_lowrank_line(FILE* f, const LowRankLineCall& c) {
  const double* o = c.o;
  fprintf(f, " \"lowrank_line\": {\"sigma\": %.17g, \"t_max\": ", c.sigma);
  if (std::isfinite(c.t_max)) fprintf(f, "%.17g", c.t_max); else fprintf(f, "null");
  fprintf(f, ", \"rmax\": %d, \"y\": %s, \"coef\": [%.17g, %.17g, %.17g, %.17g, %.17g], \"t\": %.17g, \"f\": %.17g, \"decrease\": %.17g, \"pnorm\": %.17g, "
          "\"qnorm\": %.17g, \"critical\": %.0f, \"ms\": %.17g, \"bytes\": %.0f}", c.rmax, c.have_y ? "true" : "false", c.coef[0], c.coef[1], c.coef[2], c.coef[3],
          c.coef[4], o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]);
}
// --lowrank-refine: the factors, y (when DIR/y.txt exists), sigma, steps, t_max and the results of cuadmm_lowrank_refine
struct LowRankRefineCall {
  bool on = false, have_y = false;
  int rmax = 1, steps = 10;
  double sigma = 1, t_max = INFINITY;
  std::string dir;
  std::vector<int> ranks;
  std::vector<double> L, y, trace;
  double o[8] = {0};
  int rows() const { return (int)o[0] + (o[1] != 0 ? 1 : 0); }
};
// a double as JSON: null where it is not finite
static void write_num(FILE* f, double x) { if (std::isfinite(x)) fprintf(f, "%.17g", x); else fprintf(f, "null"); }
// "lowrank_refine": {...} with the eight numbers of cuadmm_lowrank_refine and the trace's rows (t_max: null for inf)
static void write_lowrank_refine(FILE* f, const LowRankRefineCall& c) {
  fprintf(f, " \"lowrank_refine\": {\"sigma\": %.17g, \"max_steps\": %d, \"t_max\": ", c.sigma, c.steps);
  write_num(f, c.t_max);
  fprintf(f, ", \"rmax\": %d, \"y\": %s, \"steps\": %.0f, \"reason\": %.0f, \"f0\": ", c.rmax, c.have_y ? "true" : "false", c.o[0], c.o[1]);
  write_num(f, c.o[2]);
  fprintf(f, ", \"f\": ");
  write_num(f, c.o[3]);
  fprintf(f, ", \"gnorm\": ");
  write_num(f, c.o[4]);
  fprintf(f, ", \"ms\": %.17g, \"bytes\": %.0f, \"trace\": [", c.o[5], c.o[6]);
  for (int k = 0; k < c.rows(); ++k) {
    fprintf(f, "%s[", k ? ", " : "");
    for (int j = 0; j < 14; ++j) { if (j) fprintf(f, ", "); write_num(f, c.trace[16 * (size_t)k + j]); }
    fprintf(f, "]");
  }
  fprintf(f, "]}");
}
// <dir/>name.txt, one number per line (cuadmm_write_dense_txt); a missing file: zeros
static bool read_point_vec(const std::string& fn, std::vector<double>& out, size_t n, const char* who = "--kkt-point") {
  out.assign(n, 0.0);
  FILE* f = fopen(fn.c_str(), "r");
  if (!f) return true;
  size_t got = 0;
  double x = 0;
  while (got < n && fscanf(f, "%lf", &x) == 1) out[got++] = x;
  const bool more = fscanf(f, "%lf", &x) == 1;
  fclose(f);
  if (got != n || more) { std::cerr << who << ": '" << fn << "' must hold " << n << " numbers" << std::endl; return false; }
  return true;
}

// --json=<file>: one object; every number printed with %.17g
static bool write_sidecar(const std::string& path, const std::string& prefix, cuadmm_solver* solver, const cuadmm_problem_view& v, bool have_bounds,
                          const double* kkt = nullptr, const std::vector<double>& kkt_blocks = std::vector<double>(), int lm_steps = 0,
                          const double (*lm)[8] = nullptr, const LowRankReport* lr = nullptr, const LowRankStart* start = nullptr,
                          const std::vector<BlockMultCall>* bmc = nullptr, const LowRankGradCall* lgc = nullptr,
                          const LowRankLineCall* llc = nullptr, const LowRankRefineCall* lrc = nullptr) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) return false;
  const int iters = cuadmm_get_info_iter_num(solver);
  const double total_s = cuadmm_get_total_time(solver);
  double st[12] = {0}, prof[3 * CUADMM_NUM_KCLASS] = {0}, cnt[8] = {0};
  cuadmm_get_state(solver, st);
  cuadmm_get_profile(solver, prof);
  cuadmm_get_counters(solver, cnt);
  double sum_n3 = 0;
  for (int k = 0; k < v.mat_num; ++k) { const double n = v.blk_vals[k] > 0 ? v.blk_vals[k] : 0; sum_n3 += n * n * n; }
  static const char* kname[CUADMM_NUM_KCLASS] = {"aty_xb", "psd_project", "post_proj", "spmv_A", "copies", "host_solve", "allreduce", "solve_gpu_part"};
  fprintf(f, "{\n \"problem\": \"%s\",\n \"vec_len\": %d, \"con_num\": %d, \"mat_num\": %d, \"At_nnz\": %d,\n", prefix.c_str(), v.vec_len, v.con_num, v.mat_num, v.At_nnz);
  fprintf(f, " \"iterations\": %d, \"total_time_s\": %.17g, \"iters_per_s\": %.17g,\n", iters, total_s, total_s > 0 ? iters / total_s : 0.0);
  fprintf(f, " \"errRp\": %.17g, \"errRd\": %.17g, \"pobj\": %.17g, \"dobj\": %.17g, \"relgap\": %.17g, \"sig\": %.17g, \"bscale\": %.17g, \"Cscale\": %.17g,\n",
          st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]);
  fprintf(f, " \"eig_not_converged\": %.17g,\n", st[11]);
  fprintf(f, " \"plan\": {\"fused\": %d, \"closed_blocks\": %d, \"device_solve\": %d, \"factor_gpu_tail\": %d, \"batched_launches\": %.0f, \"iterations_in_batches\": %.0f},\n",
          (int)cnt[4], (int)cnt[5], (int)cnt[6], (int)cnt[7], cnt[0], cnt[1]);
  double fin[8] = {0};
  cuadmm_get_status(solver, fin);
  static const char* sname[6] = {"none", "converged", "iteration_limit", "primal_infeasible", "dual_infeasible", "certified_gap"};
  const int code = fin[0] >= 0 && fin[0] <= 5 ? (int)fin[0] : 0;
  fprintf(f, " \"status\": \"%s\", \"status_iteration\": %.0f,\n", sname[code], fin[1]);
  if (fin[2] > 0 || code == 3 || code == 4)
    fprintf(f, " \"infeas\": {\"checks\": %.0f, \"scalar\": %.17g, \"eta\": %.17g, \"radius\": %s%.17g%s, \"check_ms\": %.17g, \"bytes\": %.0f},\n", fin[2], fin[3], fin[4],
            std::isfinite(fin[5]) ? "" : "\"", fin[5], std::isfinite(fin[5]) ? "" : "\"", fin[6], fin[7]);
  if (have_bounds) {
    double lb[8] = {0}, gi[8] = {0};
    if (cuadmm_lower_bound(solver, lb, nullptr) == CUADMM_OK) {
      cuadmm_get_gap_info(solver, gi);
      fprintf(f, " \"lower_bound\": %.17g, \"certified_gap\": %.17g, \"lower_bound_parts\": {\"bty\": %.17g, \"penalty\": %.17g, \"worst_block\": %.0f, \"worst_term\": %.17g, \"ms\": %.17g},\n",
              lb[0], lb[3], lb[1], lb[2], lb[4], lb[5], lb[6]);
      if (gi[0] > 0)
        fprintf(f, " \"gap_check\": {\"checks\": %.0f, \"best_lower_bound\": %.17g, \"best_iteration\": %.0f, \"last_gap\": %.17g, \"check_ms\": %.17g, \"bytes\": %.0f, \"verdict_iteration\": %.0f},\n",
                gi[0], gi[1], gi[2], gi[4], gi[5], gi[6], gi[7]);
    } else std::cerr << cuadmm_last_error() << std::endl;
  }
  if (kkt) { write_kkt(f, kkt, kkt_blocks); fprintf(f, ",\n"); }
  if (lm) { write_lambda_min(f, lm_steps, lm); fprintf(f, ",\n"); }
  if (lr) { write_lowrank(f, *lr); fprintf(f, ",\n"); }
  if (start) { write_start(f, *start); fprintf(f, ",\n"); }
  if (bmc) { write_block_mult(f, *bmc); fprintf(f, ",\n"); }
  if (lgc) { write_lowrank_grad(f, *lgc); fprintf(f, ",\n"); }
  if (llc) { write_lowrank_line(f, *llc); fprintf(f, ",\n"); }
  if (lrc) { write_lowrank_refine(f, *lrc); fprintf(f, ",\n"); }
  double acc[8] = {0};
  cuadmm_get_accel_info(solver, acc);
  if (acc[0] > 0)
    fprintf(f, " \"accel\": {\"memory\": %.0f, \"taken\": %.0f, \"accepted\": %.0f, \"rejected\": %.0f, \"restarts\": %.0f},\n", acc[0], acc[1], acc[2], acc[3], acc[4]);
  fprintf(f, " \"phases\": {");
  for (int k = 0; k < CUADMM_NUM_KCLASS; ++k) {
    const double launches = prof[3 * k], ms = prof[3 * k + 1], bytes = prof[3 * k + 2];
    fprintf(f, "%s\n  \"%s\": {\"launches\": %.0f, \"ms\": %.17g, \"algorithmic_bytes_per_launch\": %.17g, \"gb_per_s\": %.17g}", k ? "," : "", kname[k], launches, ms,
            bytes, ms > 0 ? bytes * launches / ms * 1e-6 : 0.0);
  }
  // the projection: one launch group per iteration, 10.67 n^3 nominal flops per block
  const double pl = prof[3 * 1], pms = prof[3 * 1 + 1];
  fprintf(f, "\n },\n \"psd_project_nominal_tflops\": %.17g\n}\n", pms > 0 ? 32.0 / 3.0 * sum_n3 * pl / pms * 1e-9 : 0.0);
  return fclose(f) == 0;
}

// b.txt / C.txt of a --then stage; absent: nnz = -1 (unchanged)
static bool read_then_vec(const std::string& fn, std::vector<int>& idx, std::vector<double>& vals, int& nnz) {
  nnz = -1;
  FILE* f = fopen(fn.c_str(), "r");
  if (!f) return true;
  fclose(f);
  const int n = cuadmm_read_sparse_vec_txt(fn.c_str(), nullptr, nullptr, 0);
  if (n < 0) return false;
  idx.assign((size_t)n + 1, 0); vals.assign((size_t)n + 1, 0.0);
  nnz = cuadmm_read_sparse_vec_txt(fn.c_str(), idx.data(), vals.data(), n);
  return nnz == n;
}

int main(int argc, char* argv[]) {
  if (argc < 2) {
    std::cerr << "usage: cuadmm_exe <problem_dir/> [--key=value ...]" << std::endl;
    return 1;
  }
  std::string prefix = argv[1];
  int eig_stream_num_per_gpu = 15, cpu_eig_thread_num = 30;
  double max_iter = 1e6, stop_tol = 1e-3, threshold = 0, stage1 = 50, stage2 = 100, switch_admm = 5000, sigscale = 1.05,
         sig = 1e0, device = 0, accel = 0, infeas = 0, infeas_tol = -1, gap = 0, gap_tol = -1;
  bool quiet = false, kkt = false;
  int lm_steps = 0;      // --lambda-min: 0 = off
  LowRankReport lr;      // --lowrank: rmax = 0 = off
  bool lr_on = false;
  std::string json_path, bounds_arg, kkt_point, lr_out, start_dir, bm_out, lg_out;
  LowRankGradCall lgc;                 // --lowrank-grad
  LowRankLineCall llc;                 // --lowrank-line
  LowRankRefineCall lrc;               // --lowrank-refine
  std::string lrc_out;                 // --lowrank-refine-out
  std::vector<BlockMultCall> bmc;      // --block-mult, in the order given
  std::vector<std::string> then_dirs;
  std::vector<char> then_is_A;
  for (int i = 2; i < argc; ++i) {
    if (strncmp(argv[i], "--json=", 7) == 0) { json_path = argv[i] + 7; continue; }
    if (strncmp(argv[i], "--trace-bounds=", 15) == 0) { bounds_arg = argv[i] + 15; continue; }
    if (strncmp(argv[i], "--then=", 7) == 0) { then_dirs.push_back(argv[i] + 7); then_is_A.push_back(0); continue; }
    if (strncmp(argv[i], "--then-A=", 9) == 0) { then_dirs.push_back(argv[i] + 9); then_is_A.push_back(1); continue; }
    if (opt(argv[i], "--max_iter", max_iter) || opt(argv[i], "--stop_tol", stop_tol) || opt(argv[i], "--threshold", threshold) ||
        opt(argv[i], "--stage1", stage1) || opt(argv[i], "--stage2", stage2) || opt(argv[i], "--switch_admm", switch_admm) ||
        opt(argv[i], "--sigscale", sigscale) || opt(argv[i], "--sig", sig) || opt(argv[i], "--device", device) || opt(argv[i], "--accel", accel) ||
        opt(argv[i], "--infeas_tol", infeas_tol) || opt(argv[i], "--infeas", infeas) || opt(argv[i], "--gap_tol", gap_tol) || opt(argv[i], "--gap", gap))
      continue;
    if (strcmp(argv[i], "--quiet") == 0) { quiet = true; continue; }
    if (strcmp(argv[i], "--kkt") == 0) { kkt = true; continue; }
    if (strncmp(argv[i], "--kkt-point=", 12) == 0) { kkt_point = argv[i] + 12; continue; }
    if (strcmp(argv[i], "--lambda-min") == 0) { lm_steps = 12; continue; }
    if (strncmp(argv[i], "--lambda-min=", 13) == 0) {
      lm_steps = atoi(argv[i] + 13);
      if (lm_steps < 1 || lm_steps > 40) { std::cerr << "--lambda-min: 1 to 40 bisection steps" << std::endl; return 1; }
      continue;
    }
    if (strncmp(argv[i], "--lowrank=", 10) == 0) {
      char* end = nullptr;
      lr.tol = strtod(argv[i] + 10, &end);
      lr.rmax = 0;      // 0: the largest block size, known once the problem is read
      if (end && *end == ',') lr.rmax = atoi(end + 1);
      if (end == argv[i] + 10 || !(lr.tol >= 0 && lr.tol < 1) || (*end == ',' && lr.rmax < 1) || (*end != ',' && *end != 0)) {
        std::cerr << "--lowrank=TOL[,RMAX]: 0 <= TOL < 1, RMAX >= 1" << std::endl;
        return 1;
      }
      lr_on = true;
      continue;
    }
    if (strncmp(argv[i], "--lowrank-out=", 14) == 0) { lr_out = argv[i] + 14; continue; }
    if (strncmp(argv[i], "--start-lowrank=", 16) == 0) { start_dir = argv[i] + 16; continue; }
    if (strncmp(argv[i], "--block-mult=", 13) == 0) {
      const char* a = argv[i] + 13;
      const char* comma = strchr(a, ',');
      BlockMultCall c;
      c.which = -1;
      for (int w = 0; comma && w < 3; ++w)
        if (std::string(a, comma) == lm_names[w]) c.which = w;
      if (c.which < 0 || !comma[1]) { std::cerr << "--block-mult=X|S|dual,DIR/" << std::endl; return 1; }
      c.dir = comma + 1;
      bmc.push_back(c);
      continue;
    }
    if (strncmp(argv[i], "--block-mult-out=", 17) == 0) { bm_out = argv[i] + 17; continue; }
    if (strncmp(argv[i], "--lowrank-grad-out=", 19) == 0) { lg_out = argv[i] + 19; continue; }
    if (strncmp(argv[i], "--lowrank-grad=", 15) == 0) {
      const char* a = argv[i] + 15;
      const char* comma = strchr(a, ',');
      lgc.dir = comma ? std::string(a, comma) : std::string(a);
      char* end = nullptr;
      if (comma) lgc.sigma = strtod(comma + 1, &end);
      if (lgc.dir.empty() || (comma && (end == comma + 1 || *end != 0 || !(lgc.sigma >= 0) || !std::isfinite(lgc.sigma)))) {
        std::cerr << "--lowrank-grad=DIR/[,SIGMA]: SIGMA >= 0" << std::endl;
        return 1;
      }
      lgc.on = true;
      continue;
    }
    if (strncmp(argv[i], "--lowrank-line=", 15) == 0) {
      std::vector<std::string> part(1);
      for (const char* a = argv[i] + 15; *a; ++a)
        if (*a == ',') part.emplace_back(); else part.back() += *a;
      bool ok = part.size() >= 2 && part.size() <= 4 && !part[0].empty() && !part[1].empty();
      char* end = nullptr;
      if (ok && part.size() >= 3) { llc.sigma = strtod(part[2].c_str(), &end); ok = !part[2].empty() && *end == 0 && llc.sigma >= 0 && std::isfinite(llc.sigma); }
      if (ok && part.size() == 4) { llc.t_max = strtod(part[3].c_str(), &end); ok = !part[3].empty() && *end == 0 && !std::isnan(llc.t_max); }
      if (!ok) { std::cerr << "--lowrank-line=LDIR/,DDIR/[,SIGMA[,TMAX]]: SIGMA >= 0, TMAX a number" << std::endl; return 1; }
      llc.ldir = part[0]; llc.ddir = part[1];
      llc.on = true;
      continue;
    }
    if (strncmp(argv[i], "--lowrank-refine-out=", 21) == 0) { lrc_out = argv[i] + 21; continue; }
    if (strncmp(argv[i], "--lowrank-refine=", 17) == 0) {
      std::vector<std::string> part(1);
      for (const char* a = argv[i] + 17; *a; ++a)
        if (*a == ',') part.emplace_back(); else part.back() += *a;
      bool ok = part.size() <= 4 && !part[0].empty();
      char* end = nullptr;
      if (ok && part.size() >= 2) { lrc.sigma = strtod(part[1].c_str(), &end); ok = !part[1].empty() && *end == 0 && lrc.sigma >= 0 && std::isfinite(lrc.sigma); }
      if (ok && part.size() >= 3) { const long q = strtol(part[2].c_str(), &end, 10); ok = !part[2].empty() && *end == 0 && q >= 1 && q <= 1000000; lrc.steps = (int)q; }
      if (ok && part.size() == 4) { lrc.t_max = strtod(part[3].c_str(), &end); ok = !part[3].empty() && *end == 0 && lrc.t_max > 0; }
      if (!ok) { std::cerr << "--lowrank-refine=DIR/[,SIGMA[,STEPS[,TMAX]]]: SIGMA >= 0, STEPS >= 1, TMAX > 0" << std::endl; return 1; }
      lrc.dir = part[0];
      lrc.on = true;
      continue;
    }
    std::cerr << "unknown option " << argv[i] << std::endl;
    return 1;
  }

  if (!lr_out.empty() && !lr_on) { std::cerr << "--lowrank-out needs --lowrank=TOL[,RMAX]" << std::endl; return 1; }
  if (!bm_out.empty() && bmc.empty()) { std::cerr << "--block-mult-out needs --block-mult=X|S|dual,DIR/" << std::endl; return 1; }
  if (!lg_out.empty() && !lgc.on) { std::cerr << "--lowrank-grad-out needs --lowrank-grad=DIR/[,SIGMA]" << std::endl; return 1; }
  if (!lrc_out.empty() && !lrc.on) { std::cerr << "--lowrank-refine-out needs --lowrank-refine=DIR/[,SIGMA[,STEPS[,TMAX]]]" << std::endl; return 1; }
  for (size_t k = 0; k < then_dirs.size(); ++k) {   // before any work: a stage that cannot be read must not cost the stages before it
    const std::string& d = then_dirs[k];
    DIR* dp = d.empty() ? nullptr : opendir(d.c_str());
    if (!dp) { std::cerr << "cannot read " << (then_is_A[k] ? "--then-A" : "--then") << " directory '" << d << "'" << std::endl; return 1; }
    closedir(dp);
  }

  cuadmm_problem* prob = nullptr;
  if (cuadmm_problem_from_txt(prefix.c_str(), &prob) != CUADMM_OK) {
    std::cerr << cuadmm_last_error() << std::endl;
    return 1;   // the reference exit(1)s on unreadable input (io.cu:30-33, problem.cu:33-35)
  }
  cuadmm_problem_view v;
  cuadmm_problem_view_get(prob, &v);

  LowRankStart start;      // --start-lowrank: read and checked before any device work
  if (!start_dir.empty()) {
    FILE* yf = fopen((start_dir + "y.txt").c_str(), "r");
    if (yf) { fclose(yf); start.have_y = true; }
    if (!read_lowrank_start(start_dir, v, start) || (start.have_y && !read_point_vec(start_dir + "y.txt", start.y, (size_t)v.con_num, "--start-lowrank"))) {
      cuadmm_problem_free(prob);
      return 1;
    }
  }

  for (auto& c : bmc)      // --block-mult: read and checked before any device work
    if (!read_block_mult(v, c)) { cuadmm_problem_free(prob); return 1; }

  if (lgc.on) {            // --lowrank-grad: read and checked before any device work
    LowRankStart st;
    bool ok = read_lowrank_start(lgc.dir, v, st, 0) && (st.have[0] || read_lowrank_start(lgc.dir, v, st, 1));
    const int w = st.have[0] ? 0 : 1;
    if (ok && !st.have[w]) { std::cerr << "--lowrank-grad: no factor file L_X_<k>.txt or L_S_<k>.txt in '" << lgc.dir << "'" << std::endl; ok = false; }
    FILE* yf = ok ? fopen((lgc.dir + "y.txt").c_str(), "r") : nullptr;
    if (yf) { fclose(yf); lgc.have_y = true; }
    if (ok && lgc.have_y) ok = read_point_vec(lgc.dir + "y.txt", lgc.y, (size_t)v.con_num, "--lowrank-grad");
    if (!ok) { cuadmm_problem_free(prob); return 1; }
    lgc.rmax = st.rmax[w]; lgc.ranks = st.ranks[w]; lgc.L = st.L[w];
    lgc.G.assign(lgc.L.size(), 0.0);
    lgc.r.assign((size_t)v.con_num + 1, 0.0);
  }

  if (llc.on) {            // --lowrank-line: read and checked before any device work
    LowRankStart sl, sd;
    bool ok = read_lowrank_start(llc.ldir, v, sl, 0) && (sl.have[0] || read_lowrank_start(llc.ldir, v, sl, 1));
    ok = ok && read_lowrank_start(llc.ddir, v, sd, 0) && (sd.have[0] || read_lowrank_start(llc.ddir, v, sd, 1));
    const int wl = sl.have[0] ? 0 : 1, wd = sd.have[0] ? 0 : 1;
    if (ok && (!sl.have[wl] || !sd.have[wd])) {
      std::cerr << "--lowrank-line: no factor file L_X_<k>.txt or L_S_<k>.txt in '" << (sl.have[wl] ? llc.ddir : llc.ldir) << "'" << std::endl;
      ok = false;
    }
    if (ok && sl.ranks[wl] != sd.ranks[wd]) { std::cerr << "--lowrank-line: the direction's ranks are not the factors'" << std::endl; ok = false; }
    FILE* yf = ok ? fopen((llc.ldir + "y.txt").c_str(), "r") : nullptr;
    if (yf) { fclose(yf); llc.have_y = true; }
    if (ok && llc.have_y) ok = read_point_vec(llc.ldir + "y.txt", llc.y, (size_t)v.con_num, "--lowrank-line");
    if (!ok) { cuadmm_problem_free(prob); return 1; }
    llc.rmax = sl.rmax[wl]; llc.ranks = sl.ranks[wl]; llc.L = sl.L[wl]; llc.D = sd.L[wd];   // (equal ranks: equal rmax, one layout)
  }

  if (lrc.on) {            // --lowrank-refine: read and checked before any device work
    LowRankStart st;
    bool ok = read_lowrank_start(lrc.dir, v, st, 0) && (st.have[0] || read_lowrank_start(lrc.dir, v, st, 1));
    const int w = st.have[0] ? 0 : 1;
    if (ok && !st.have[w]) { std::cerr << "--lowrank-refine: no factor file L_X_<k>.txt or L_S_<k>.txt in '" << lrc.dir << "'" << std::endl; ok = false; }
    FILE* yf = ok ? fopen((lrc.dir + "y.txt").c_str(), "r") : nullptr;
    if (yf) { fclose(yf); lrc.have_y = true; }
    if (ok && lrc.have_y) ok = read_point_vec(lrc.dir + "y.txt", lrc.y, (size_t)v.con_num, "--lowrank-refine");
    if (!ok) { cuadmm_problem_free(prob); return 1; }
    lrc.rmax = st.rmax[w]; lrc.ranks = st.ranks[w]; lrc.L = st.L[w];
    lrc.trace.assign(16 * (size_t)lrc.steps, 0.0);
  }

  cuadmm_solver* solver = nullptr;
  cuadmm_create(&solver);
  cuadmm_set_option(solver, "device", device);
  cuadmm_set_option(solver, "verbose", quiet ? 0 : 1);
  if (!json_path.empty()) cuadmm_set_option(solver, "profile", 1);
  if (accel != 0 && cuadmm_set_option(solver, "accel", accel) != CUADMM_OK) {
    std::cerr << cuadmm_last_error() << std::endl;
    return 1;
  }
  if ((infeas != 0 && cuadmm_set_option(solver, "infeas_check", infeas) != CUADMM_OK) ||
      (infeas_tol >= 0 && cuadmm_set_option(solver, "infeas_tol", infeas_tol) != CUADMM_OK)) {
    std::cerr << cuadmm_last_error() << std::endl;
    return 1;
  }
  if (!bounds_arg.empty()) {
    std::vector<double> R((size_t)v.mat_num, -1.0);
    if (bounds_arg == "auto") {
      if (cuadmm_trace_bounds_detect(v.vec_len, v.con_num, v.At_csc_col_ptrs, v.At_csc_row_ids, v.At_csc_vals, v.b_indices, v.b_vals, v.b_nnz, v.blk_vals,
                                     v.mat_num, R.data()) != CUADMM_OK) {
        std::cerr << cuadmm_last_error() << std::endl;
        return 1;
      }
      for (int k = 0; k < v.mat_num; ++k)
        if (R[k] < 0) { std::cerr << "--trace-bounds=auto: the constraints give no bound for block " << k << " (size " << v.blk_vals[k] << ")" << std::endl; return 1; }
    } else {
      FILE* bf = fopen(bounds_arg.c_str(), "r");
      int got = 0;
      double x = 0;
      while (bf && got < v.mat_num && fscanf(bf, "%lf", &x) == 1) R[got++] = x;
      const bool more = bf && fscanf(bf, "%lf", &x) == 1;
      if (bf) fclose(bf);
      if (!bf || got != v.mat_num || more) { std::cerr << "--trace-bounds: '" << bounds_arg << "' must hold " << v.mat_num << " numbers, one per block" << std::endl; return 1; }
    }
    if (cuadmm_set_trace_bounds(solver, R.data(), v.mat_num) != CUADMM_OK) { std::cerr << cuadmm_last_error() << std::endl; return 1; }
  }
  if ((gap != 0 && cuadmm_set_option(solver, "gap_check", gap) != CUADMM_OK) || (gap_tol >= 0 && cuadmm_set_option(solver, "gap_tol", gap_tol) != CUADMM_OK)) {
    std::cerr << cuadmm_last_error() << std::endl;
    return 1;
  }
  int rc = cuadmm_init(solver, eig_stream_num_per_gpu, cpu_eig_thread_num, v.vec_len, v.con_num, v.At_csc_col_ptrs,
                       v.At_csc_row_ids, v.At_csc_vals, v.At_nnz, v.b_indices, v.b_vals, v.b_nnz, v.C_indices, v.C_vals,
                       v.C_nnz, v.blk_vals, v.mat_num, nullptr, nullptr, nullptr, sig);
  if (rc != CUADMM_OK) {
    std::cerr << cuadmm_last_error() << std::endl;
    return 1;
  }
  double kk[16] = {0};
  std::vector<double> kkb(6 * (size_t)v.mat_num);
  if (!kkt_point.empty()) {       // the report of a point from files, no solve
    std::vector<double> pX, py, pS;
    rc = (read_point_vec(kkt_point + "X.txt", pX, (size_t)v.vec_len) && read_point_vec(kkt_point + "y.txt", py, (size_t)v.con_num) &&
          read_point_vec(kkt_point + "S.txt", pS, (size_t)v.vec_len)) ? CUADMM_OK : CUADMM_ERR_IO;
    if (rc == CUADMM_OK && (rc = cuadmm_evaluate(solver, pX.data(), py.data(), pS.data(), kk, kkb.data())) != CUADMM_OK) std::cerr << cuadmm_last_error() << std::endl;
    if (rc == CUADMM_OK) {
      print_kkt(kk, kkb);
      if (!json_path.empty()) {
        FILE* f = fopen(json_path.c_str(), "w");
        if (f) { fprintf(f, "{\n \"problem\": \"%s\", \"point\": \"%s\",\n", prefix.c_str(), kkt_point.c_str()); write_kkt(f, kk, kkb); fprintf(f, "\n}\n"); }
        if (!f || fclose(f) != 0) std::cerr << "cannot write " << json_path << std::endl;
      }
    }
    cuadmm_destroy(solver);
    cuadmm_problem_free(prob);
    return rc == CUADMM_OK ? 0 : 1;
  }
  // --kkt: the report of the point a solve returns, taken before anything reads the iterate
  auto kkt_report = [&]() {
    if (!kkt) return false;
    if (cuadmm_evaluate(solver, nullptr, nullptr, nullptr, kk, kkb.data()) != CUADMM_OK) { std::cerr << cuadmm_last_error() << std::endl; return false; }
    print_kkt(kk, kkb);
    return true;
  };
  // --lambda-min: the certified bounds at the point a solve returns, taken before anything reads the iterate
  double lm[3][8] = {{0}};
  auto lm_report = [&]() {
    if (lm_steps == 0) return false;
    for (int w = 0; w < 3; ++w) {
      if (cuadmm_lambda_min(solver, w, lm_steps, lm[w], nullptr) != CUADMM_OK) { std::cerr << cuadmm_last_error() << std::endl; return false; }
      printf(" lambda_min(%s) >= %.10e (block %.0f), DIMACS measure <= %.3e, %.0f unrefined, %.0f PSD at the floor, %.3f ms", lm_names[w], lm[w][0], lm[w][1],
             lm[w][2], lm[w][4], lm[w][5], lm[w][6]);
      if (std::isfinite(lm[w][3])) printf(", LB_lambda = %.10e", lm[w][3]);
      printf("\n");
    }
    return true;
  };
  // --lowrank: ranks (and, with --lowrank-out, factors) at the point a solve returns, taken before anything reads the iterate
  auto lr_report = [&]() {
    if (!lr_on) return false;
    if (lr.rmax == 0)
      for (int k = 0; k < v.mat_num; ++k) lr.rmax = std::max(lr.rmax, std::max(v.blk_vals[k], 1));
    long long count = 0;
    if (cuadmm_lowrank_size(solver, lr.rmax, &count) != CUADMM_OK) { std::cerr << cuadmm_last_error() << std::endl; return false; }
    for (int w = 0; w < 2; ++w) {
      lr.pb[w].assign(6 * (size_t)v.mat_num, 0.0);
      if (!lr_out.empty()) lr.L[w].assign((size_t)count + 1, 0.0);
      if (cuadmm_lowrank(solver, w, lr.tol, lr.rmax, lr.o[w], lr.pb[w].data(), lr_out.empty() ? nullptr : lr.L[w].data(), nullptr) != CUADMM_OK) {
        std::cerr << cuadmm_last_error() << std::endl;
        return false;
      }
      printf(" rank(%s): sum %.0f, max %.0f (block %.0f), residual trace %.3e, min residual diagonal %.3e, %.0f stopped at %d columns, %.3f ms\n", lm_names[w],
             lr.o[w][0], lr.o[w][1], lr.o[w][2], lr.o[w][3], lr.o[w][4], lr.o[w][5], lr.rmax, lr.o[w][6]);
      for (int k = 0; k < v.mat_num && !lr_out.empty(); ++k) {
        const double* q = lr.pb[w].data() + 6 * (size_t)k;
        if (v.blk_vals[k] <= 0) continue;
        const std::string fn = lr_out + "L_" + lm_names[w] + "_" + std::to_string(k) + ".txt";
        if (cuadmm_write_dense_txt(fn.c_str(), lr.L[w].data() + (size_t)q[5], (int64_t)v.blk_vals[k] * (int64_t)q[0]) != CUADMM_OK) {
          std::cerr << cuadmm_last_error() << std::endl;
          return false;
        }
      }
    }
    return true;
  };
  // --block-mult: the products at the point a solve returns, taken before anything reads the iterate
  auto bm_report = [&]() {
    for (auto& c : bmc) {
      if (cuadmm_block_multiply(solver, c.which, c.V.data(), c.ranks.data(), c.rmax, c.W.data(), c.o, nullptr) != CUADMM_OK) { std::cerr << cuadmm_last_error() << std::endl; return false; }
      printf(" block_mult(%s): ||W||_F = %.10e, <V, W> = %.10e, largest block %.0f (%.3e), %.0f blocks, rank sum %.0f, %.3f ms\n", lm_names[c.which], c.o[0], c.o[1],
             c.o[2], c.o[3], c.o[4], c.o[5], c.o[6]);
      size_t at = 0;
      for (int k = 0; k < v.mat_num && !bm_out.empty(); ++k) {
        const long long n = v.blk_vals[k];
        if (n <= 0) continue;
        const std::string fn = bm_out + "W_" + std::to_string(k) + ".txt";
        FILE* f = fopen(fn.c_str(), "w");
        if (!f) { std::cerr << "cannot write " << fn << std::endl; return false; }
        for (long long e = 0; e < n * c.ranks[k]; ++e) fprintf(f, "%.17g\n", c.W[at + (size_t)e]);
        fclose(f);
        at += (size_t)(n * std::min<long long>(n, c.rmax));
      }
    }
    return !bmc.empty();
  };
  // --lowrank-grad: value and gradient at the point a solve returns, taken before anything reads the iterate
  auto lg_report = [&]() {
    if (!lgc.on) return false;
    LowRankGradCall& c = lgc;
    if (cuadmm_lowrank_grad(solver, c.L.data(), c.ranks.data(), c.rmax, c.have_y ? c.y.data() : nullptr, c.sigma, c.G.data(), c.r.data(), nullptr, c.o, nullptr) != CUADMM_OK) {
      std::cerr << cuadmm_last_error() << std::endl;
      return false;
    }
    printf(" lowrank_grad(sigma = %g): f = %.10e, <C, x> = %.10e, y'r = %.10e, ||r|| = %.10e, ||G||_F = %.10e, <L, G> = %.10e, %.3f ms\n", c.sigma, c.o[0], c.o[1], c.o[2],
           c.o[3], c.o[4], c.o[5], c.o[6]);
    if (lg_out.empty()) return true;
    size_t at = 0;
    for (int k = 0; k < v.mat_num; ++k) {
      const long long n = v.blk_vals[k];
      if (n <= 0) continue;
      const std::string fn = lg_out + "G_" + std::to_string(k) + ".txt";
      FILE* f = fopen(fn.c_str(), "w");
      if (!f) { std::cerr << "cannot write " << fn << std::endl; return false; }
      for (long long e = 0; e < n * c.ranks[k]; ++e) fprintf(f, "%.17g\n", c.G[at + (size_t)e]);
      fclose(f);
      at += (size_t)(n * std::min<long long>(n, c.rmax));
    }
    FILE* f = fopen((lg_out + "r.txt").c_str(), "w");
    if (!f) { std::cerr << "cannot write " << lg_out << "r.txt" << std::endl; return false; }
    for (int i = 0; i < v.con_num; ++i) fprintf(f, "%.17g\n", c.r[(size_t)i]);
    fclose(f);
    return true;
  };
  // --lowrank-line: the quartic along the direction at the point a solve returns, taken before anything reads the iterate
  auto ll_report = [&]() {
    if (!llc.on) return false;
    LowRankLineCall& c = llc;
    if (cuadmm_lowrank_line(solver, c.L.data(), c.D.data(), c.ranks.data(), c.rmax, c.have_y ? c.y.data() : nullptr, c.sigma, c.t_max, c.coef, nullptr, nullptr, nullptr,
                            c.o, nullptr) != CUADMM_OK) {
      std::cerr << cuadmm_last_error() << std::endl;
      return false;
    }
    printf(" lowrank_line(sigma = %g, t_max = %g): c = [%.10e, %.10e, %.10e, %.10e, %.10e], t* = %.10e, f(t*) = %.10e, %.3f ms\n", c.sigma, c.t_max, c.coef[0],
           c.coef[1], c.coef[2], c.coef[3], c.coef[4], c.o[0], c.o[1], c.o[6]);
    return true;
  };
  // --lowrank-refine: conjugate gradients over the factors at the point a solve returns, taken before anything reads the iterate; every
  // solve refines the factors that were read
  auto lrr_report = [&]() {
    if (!lrc.on) return false;
    LowRankRefineCall& c = lrc;
    std::vector<double> Lo(c.L.size(), 0.0);
    if (cuadmm_lowrank_refine(solver, c.L.data(), c.ranks.data(), c.rmax, c.have_y ? c.y.data() : nullptr, c.sigma, c.steps, c.t_max, 0.0, Lo.data(), c.trace.data(),
                              c.o, nullptr) != CUADMM_OK) {
      std::cerr << cuadmm_last_error() << std::endl;
      return false;
    }
    for (int k = 0; k < c.rows(); ++k) {
      const double* q = c.trace.data() + 16 * (size_t)k;
      printf(" lowrank_refine step %d: f = %.10e, ||G||_F = %.10e, beta = %.3e%s, t = %.10e, f(t) = %.10e, %.3f ms\n", k, q[6], std::sqrt(q[0]), q[3],
             q[5] != 0 ? " (restart)" : "", q[11], q[12], q[13]);
    }
    printf(" lowrank_refine(sigma = %g, t_max = %g): %.0f steps, reason %.0f, f %.10e -> %.10e, %.3f ms\n", c.sigma, c.t_max, c.o[0], c.o[1], c.o[2], c.o[3], c.o[5]);
    if (lrc_out.empty()) return true;
    size_t at = 0;
    for (int k = 0; k < v.mat_num; ++k) {
      const long long n = v.blk_vals[k];
      if (n <= 0) continue;
      const std::string fn = lrc_out + "L_X_" + std::to_string(k) + ".txt";
      FILE* f = fopen(fn.c_str(), "w");
      if (!f) { std::cerr << "cannot write " << fn << std::endl; return false; }
      for (long long e = 0; e < n * c.ranks[k]; ++e) fprintf(f, "%.17g\n", Lo[at + (size_t)e]);
      fclose(f);
      at += (size_t)(n * std::min<long long>(n, c.rmax));
    }
    return true;
  };
  // --start-lowrank: the point replaces init's zeros, and the solve takes the iterate as it stands (if_first = 0)
  const bool started = start.have[0] || start.have[1] || start.have_y;
  for (int w = 0; w < 2 && rc == CUADMM_OK; ++w) {
    if (!start.have[w]) continue;
    rc = cuadmm_set_lowrank(solver, w, start.L[w].data(), start.ranks[w].data(), start.rmax[w], 0.0, start.o[w]);
    if (rc == CUADMM_OK) printf(" start(%s): %.0f blocks from factors, rank sum %.0f, %.3f ms\n", lm_names[w], start.o[w][0], start.o[w][1], start.o[w][2]);
  }
  if (rc == CUADMM_OK && start.have_y) rc = cuadmm_set_XyS(solver, nullptr, start.y.data(), nullptr, 0.0);
  if (rc != CUADMM_OK) {
    std::cerr << cuadmm_last_error() << std::endl;
    cuadmm_destroy(solver);
    cuadmm_problem_free(prob);
    return 1;
  }
  rc = cuadmm_solve(solver, (int)max_iter, stop_tol, (int)threshold, (int)stage1, (int)stage2, (int)switch_admm, sigscale, started ? 0 : 1);
  if (rc != CUADMM_OK) std::cerr << cuadmm_last_error() << std::endl;
  bool have_kkt = kkt_report();
  bool have_lm = lm_report();
  bool have_lr = lr_report();
  bool have_bm = bm_report();
  bool have_lg = lg_report();
  bool have_ll = ll_report();
  bool have_lrr = lrr_report();

  if (accel != 0) {
    double acc[8] = {0};
    cuadmm_get_accel_info(solver, acc);
    printf("accel: taken %.0f, accepted %.0f, rejected %.0f, restarts %.0f\n", acc[1], acc[2], acc[3], acc[4]);
  }
  std::vector<double> X((size_t)v.vec_len);
  if (cuadmm_get_X(solver, X.data()) == CUADMM_OK) cuadmm_write_dense_txt((prefix + "X_opt.txt").c_str(), X.data(), v.vec_len);
  if (!json_path.empty() && !write_sidecar(json_path, prefix, solver, v, !bounds_arg.empty(), have_kkt ? kk : nullptr, kkb, lm_steps, have_lm ? lm : nullptr, have_lr ? &lr : nullptr, started ? &start : nullptr, have_bm ? &bmc : nullptr, have_lg ? &lgc : nullptr, have_ll ? &llc : nullptr, have_lrr ? &lrc : nullptr)) std::cerr << "cannot write " << json_path << std::endl;
  for (size_t k = 0; k < then_dirs.size() && rc == CUADMM_OK; ++k) {
    const std::string& d = then_dirs[k];
    std::vector<int> bi, ci;
    std::vector<double> bv, cv;
    int bn = -1, cn = -1;
    if (then_is_A[k]) {
      cuadmm_problem* p2 = nullptr;
      if (cuadmm_problem_from_txt(d.c_str(), &p2) != CUADMM_OK) { std::cerr << cuadmm_last_error() << std::endl; rc = CUADMM_ERR_IO; break; }
      cuadmm_problem_view w;
      cuadmm_problem_view_get(p2, &w);
      bool same = w.vec_len == v.vec_len && w.con_num == v.con_num && w.At_nnz == v.At_nnz && w.mat_num == v.mat_num;
      for (int j = 0; same && j <= v.con_num; ++j) same = w.At_csc_col_ptrs[j] == v.At_csc_col_ptrs[j];
      for (int q = 0; same && q < v.At_nnz; ++q) same = w.At_csc_row_ids[q] == v.At_csc_row_ids[q];
      for (int q = 0; same && q < v.mat_num; ++q) same = w.blk_vals[q] == v.blk_vals[q];
      if (!same) { std::cerr << "--then-A: the problem in '" << d << "' does not have the sparsity pattern of A (or the blocks) of '" << prefix << "'" << std::endl; rc = CUADMM_ERR_INVALID; }
      else rc = cuadmm_update_A(solver, w.At_csc_vals, w.At_nnz, 1, 0.0);
      cuadmm_problem_free(p2);
      if (rc != CUADMM_OK) { if (same) std::cerr << cuadmm_last_error() << std::endl; break; }
    }
    if (!read_then_vec(d + "b.txt", bi, bv, bn) || !read_then_vec(d + "C.txt", ci, cv, cn)) { std::cerr << cuadmm_last_error() << std::endl; rc = CUADMM_ERR_IO; break; }
    rc = cuadmm_update_bC(solver, bi.data(), bv.data(), bn, ci.data(), cv.data(), cn, 1, 0.0);
    if (rc == CUADMM_OK) rc = cuadmm_solve(solver, (int)max_iter, stop_tol, (int)threshold, (int)stage1, (int)stage2, (int)switch_admm, sigscale, 1);
    if (rc != CUADMM_OK) { std::cerr << cuadmm_last_error() << std::endl; break; }
    have_kkt = kkt_report();
    have_lm = lm_report();
    have_lr = lr_report();
    have_bm = bm_report();
    have_lg = lg_report();
    have_ll = ll_report();
    have_lrr = lrr_report();
    if (cuadmm_get_X(solver, X.data()) == CUADMM_OK) cuadmm_write_dense_txt((d + "X_opt.txt").c_str(), X.data(), v.vec_len);
    const std::string side = json_path + "." + std::to_string(k + 1);
    if (!json_path.empty() && !write_sidecar(side, d, solver, v, !bounds_arg.empty(), have_kkt ? kk : nullptr, kkb, lm_steps, have_lm ? lm : nullptr, have_lr ? &lr : nullptr, nullptr, have_bm ? &bmc : nullptr, have_lg ? &lgc : nullptr, have_ll ? &llc : nullptr, have_lrr ? &lrc : nullptr)) std::cerr << "cannot write " << side << std::endl;
  }
  cuadmm_destroy(solver);
  cuadmm_problem_free(prob);
  return rc == CUADMM_OK ? 0 : 1;
}
