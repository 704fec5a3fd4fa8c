// The state of one solver handle (struct cuadmm_solver) and what the engine's units share: the RCCL binding, the in-process group's
// forwarding helpers, and the routines of init that cuadmm_update_bC / cuadmm_update_A run again.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>

#include "dev_buf.h"
#include "option_table.h"
#include "report_plans.h"
#include "tail_solve.h"
#include "lead_solve.h"
#include "vec_kernels.h"
#include "duo_group.h"
#include "accel.h"
#include "infeas.h"
#include "lower_bound.h"
#include "evaluate.h"

using namespace cuadmm;      // (internal header: struct cuadmm_solver is the C API's opaque type and lives at global scope)

namespace cuadmm {
// direct RCCL binding (symbols resolved at run time so that a process that already loaded an RCCL,
// e.g. through torch, shares it)
struct NcclUid { char internal[128]; };
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(NcclUid*) = nullptr;
  int (*CommInitRank)(void**, int, NcclUid, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  bool load() {
    if (AllReduce) return true;
    void* h = dlopen(nullptr, RTLD_NOW);
    if (!h || !dlsym(h, "ncclAllReduce")) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return false;
    lib = h;
    GetUniqueId = (int (*)(NcclUid*))dlsym(h, "ncclGetUniqueId");
    CommInitRank = (int (*)(void**, int, NcclUid, int))dlsym(h, "ncclCommInitRank");
    AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclAllReduce");
    CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    return GetUniqueId && CommInitRank && AllReduce;
  }
};
extern RcclApi g_rccl;      // one per library (engine.hip)
}  // namespace cuadmm

struct cuadmm_solver {
  // options
  int device = 0, verbose = 1, rank = 0, world = 1, profile = 0, force_comm = 0, psd_steps = 0;
  // rank-limited projection (dormant in the reference: duo_solver.cu:428-438,843-850): keep only the eig_rank
  // largest eigenvalues of every PSD block from iteration eig_rank_begin_iter on, or once maxfeas < eig_rank_maxfeas
  int eig_rank = 0, eig_rank_begin_iter = 0;
  double eig_rank_maxfeas = 0.0;
  cuadmm_allreduce_fn allreduce = nullptr;
  void* allreduce_user = nullptr;
  void* rccl_comm = nullptr;

  bool initialised = false;
  hipStream_t st = nullptr;
  double t_init0 = 0, total_time = 0;

  // global dims
  int L_full = 0, m = 0, nblk_full = 0;
  // shard
  int blk_begin = 0, blk_end = 0;
  long long sv_begin = 0, sv_end = 0;
  long long L = 0;
  std::vector<int> blk_local;

  // host state (constraint space, permuted order unless noted)
  // "Owned constraints" mode of a sharded run: when every constraint touches the blocks of ONE rank only (block-diagonal
  // problems: the synthetic weak-scaling configurations), each rank keeps just its own constraints -- its own small
  // factor, its own PCIe traffic -- and the ranks exchange four scalars per iteration instead of all-reducing A*X and
  // replicating the whole solve.  world / rank are then 1 / 0 for the sharding logic, comm_world / comm_rank hold the
  // communicator, m_full / cons_local / sv_off / blk_off map back to the caller's numbering.
  bool local_mode = false;
  int comm_world = 1, comm_rank = 0, m_full = 0, blk_off = 0;
  int L_caller = 0, nblk_caller = 0;   // the caller's vec_len / mat_num (cuadmm_get_dims reports the caller's numbering)
  long long sv_off = 0;
  std::vector<int> cons_local, cons_g2l;   // this rank's constraints in the caller's numbering, and the way back (-1: another rank's)
  double ov_nb = 0, ov_nc = 0, ov_nb2 = 0;
  DevBuf<double> scal_d, yfull_d, b_d, normA_d;
  PinnedBuf<double> h_scal;
  double* h_scal_dev = nullptr;   // device mapping of h_scal
  // owned-constraints mode over > 1 ranks: the four scalars of the stopping test are formed on the device (rp_stats_kernel),
  // all-reduced on the stream and copied down with the result vector: one stream synchronisation per iteration, no
  // H2D -> collective -> D2H -> sync round trip of their own
  bool dev_scalars = false;
  // where a reduction leaves scalars for the host: the pinned buffer itself through its device mapping when no collective follows
  double* scalars_dst(double* mapped, double* dev) const { return (!dev_scalars && mapped) ? mapped : dev; }
  // Device-side y-solve (forest_solve_kernel) when the elimination forest of the factor is many small trees (block-diagonal
  // A A^T: C2, C4, ros_2000 ...): y, A X, A(S-C), b stay in HBM, the host fetches only the four scalars of the stopping test.
  bool dev_solve = false;
  // Fused iteration (psd_fuse.h): the projection kernels of the 17 <= n <= 64 blocks form Xb themselves and apply the S / X
  // updates to their svec ranges; the stand-alone vector kernels visit only the rest of the svec (plan.d_rest).
  bool fuse = false;
  // ... and the constraint rows whose nonzeros all lie in one fused block are evaluated there too (SignFuse::lc_*); the
  // stand-alone SpMV then only visits the other rows (compact CSR + the constraint index of each row)
  struct LocalRows {
    bool active = false;
    int nlocal = 0, nrest = 0;
    double rest_avg = 1.0;
    DevBuf<LcDesc> desc;
    DevBuf<int> row, nzptr, e, rest_rp, rest_ci, rest_map;
    DevBuf<double> v, rest_v;
    std::vector<LcDesc> h_desc;      // host copies for the closed-block set-up
    std::vector<int> h_row, h_nzptr, h_e;
    std::vector<double> h_v;
  } lrows;
  // closed blocks (psd_fuse.h): every constraint is local to one fused block and no block has more than kClosedMaxRows of
  // them -> the blocks solve for their own multipliers and add their share of ||Rp||^2, b^T y inside the projection kernel
  struct ClosedSolve {
    bool active = false;
    DevBuf<ClosedRec> rec;         // one record per fused slot (psd_fuse.h)
    DevBuf<double> partials2, cl_out;
    bool out_dirty = true;         // a stand-alone kernel rewrote [A X | A (S - C)] by row: refresh the per-block copy first
    long long iters_done = 0;      // fused closed iterations launched so far (ages the schedule hints deterministically)
  } closed;
  DevBuf<double> quad_seg;         // segment sums of launch_reduce_quads (more than 16 384 fused blocks)
  bool stats_fused = false;        // this iteration's four scalars were formed by launch_reduce_quads
  int fused_nparts = 0;
  // Several iterations per launch (SignFuse::iters; closed blocks, ADMM phase): option "batch" = most iterations per launch
  // (0 / 1: off).  bt_p1 / bt_p2: the per-iteration partial arrays, bt_h: the four scalars of every iteration of the batch
  // (pinned, written by the reduction through its device mapping when no collective is needed), ck_*: the checkpoint a batch
  // starts from (restored when the stopping test or the tau rule fires inside it).
  // SDPDuoSolver's N-devices-from-one-process mode (duo_group.hip): this handle is rank 0 of a group; `in_group_call` marks the
  // calls the group makes on its own ranks.  option_log: every accepted cuadmm_set_option so far but the per-rank keys (replayed on the group's children).
  void* group = nullptr;
  bool in_group_call = false;
  int duo_share_device = 0;
  int duo_exchange = -1;              // -1: device-side exchange when the ranks' devices can read each other, else host-staged
  long long duo_inject = 0;           // test hook: duo_group.hip, DuoGroup::inject
  std::vector<std::pair<std::string, double>> option_log;
  struct Batch {
    int max_iters = 64;
    bool allow_mixed = false;      // option "batch_mixed": batches although several tile geometries share the work (tests)
    DevBuf<double> p1, p2, scal_d, ck_X, ck_S, ck_y, ck_out;
    DevBuf<int> ck_hint;
    long long ck_iters_done = 0;
    PinnedBuf<double> h;
    double* h_dev = nullptr;
    long long pstride = 0;
    int cap = 0;                   // iterations the partial / scalar buffers were sized for (batch_alloc); K never exceeds it
    bool peers_agree = true;       // every rank of the communicator can batch (agreed at the start of each solve: a rank that batches
                                   // issues ONE collective of 4 K scalars per batch, a rank that does not issues one of 4 per iteration)
    int len = 0, pos = 0;          // iterations launched / consumed by the host loop
    bool have_ck = false;          // this batch started from a checkpoint (taken whenever something could invalidate it)
    double tau = 0, sig = 0;
    long long launches = 0, iters = 0, rollbacks = 0;
  } bt;
  // X, S (device) and y hold SCALED values after a solve until somebody looks at them (materialise): a second solve with
  // if_first = false then simply continues, instead of unscaling and rescaling three vectors and recomputing A X, A (S - C)
  bool pending_unscale = false;
  int lazy_unscale = 1;
  // cuadmm_update_bC rescaled y on the device (y-solve there): y_p is behind y_d until somebody on the host needs it (sync_y_host)
  bool y_host_stale = false;
  std::vector<double> normA_all;      // owned constraints: max(1, ||column||) of EVERY constraint (bscale of a new b runs over all of them)
  // cuadmm_update_A (new values of A on the pattern of init).  Kept since init: the caller's pattern of A^T and b in the caller's units
  // and entry order (b is divided by the new column norms, bscale summed in that order; cuadmm_update_bC replaces them).  Built at
  // the first update: the two index maps of the value pass (CSR slot -> position in the caller's value array) and the host's row
  // pointers of A.  factor_bad: the last update could not factor the new A A^T; solve refuses until an update succeeds.
  struct UpdateA {
    std::vector<int> cp, ri, b_idx;
    std::vector<double> b_val;
    // owned constraints: the caller's column pointers, where this rank's entries sit in the caller's value array, and the whole b
    // (the column norms of EVERY constraint and bscale over all of b are formed again from the full inputs, as in init)
    std::vector<int> g_cp, g_from, bg_idx;
    std::vector<double> bg_val;
    bool maps = false, in_update = false, tail_fellback = false;
    int inject_fail = 0;      // test hook (option "update_A_inject_fail"): the NEXT update fails as a broken factorisation would, 1: behind the
                              // host refactorisation, 2: behind the rebuilt GPU tail and y-solve streams; cleared by that update
    std::vector<int> h_fromA, h_fromAt, h_arp;
    DevBuf<int> fromA, fromAt;
    DevBuf<double> src;
    long long count = 0, orderings = 0;
    double wall_ms = 0, host_ms = 0, dev_ms = 0, bytes = 0;
    // option profile: the two streaming passes of the last update timed by events of their own (the K_COPY / K_POST classes also hold what the
    // residual stage behind them does): [0, 1] around the value pass's kernel, [2, 3] around the svec pass
    DevEvent ev[4];
    double pass_ms[2] = {0, 0}, pass_bytes[2] = {0, 0};
  } upa;
  bool factor_bad = false;
  // Behavioural switches (cuadmm_set_option, before init).  The environment variables of round 1 / 2 only give the DEFAULTS, read
  // once per solver in its constructor: two solvers in a process can choose differently, and tests reach every variant.  The keys of
  // these and of every other option of the handle, their variables and their checks: engine_option_table (option_table.h).
  struct Switches {
    int fuse = 1;                 // "fuse": the vector work of 9 <= n <= 64 blocks inside their projection kernels
    int fuse_rows = 1;            // "fuse_rows": constraint rows local to one fused block evaluated there
    int fuse_solve = -1;          // "fuse_solve": closed blocks solve for their own multipliers (-1: whenever possible)
    int host_solve = 0;           // "host_solve": keep the y-solve on the host (no forest / lead / tail on the device)
    int host_scalars = 0;         // "host_scalars": owned constraints: the four scalars through the host
    int tail_k = -1;              // "tail_k": -1 cost model, 0 host-only factor, k > 0 forces the GPU tail size
    int local_constraints = 1;    // "local_constraints": owned-constraints sharding when the problem allows it
    int mapped_out = 1;           // "mapped_out": results through a mapped pinned buffer when no collective is needed
    int lpt = 1;                  // "lpt": longest block first
    int aty_post2 = 1;            // "aty_post2": the sGS second half in one pass
    int lead_stream = 0;          // "lead_stream": the leading sweeps on the streaming kernels only (no LDS-resident trees; A/B, tests)
    int tail_one_pass = 1;        // "tail_one_pass": the GPU tail applied in one pass over inv(L22) (0: two triangular GEMVs)
    int solve_next = 1;           // "solve_next": the y-solve of iteration k + 1 is enqueued before the host waits for iteration k (fetch_out)
    int tail_max_k = 32768;       // "tail_max_k": cap of the planner's GPU tail (<= 65 536: 3 x 8 K^2 bytes while it is built, 2 x 8 K^2 afterwards)
    int tail_refine = 0;          // "tail_refine": accuracy mode of the tail (tail_solve.h)
    int tail_pivot = 1;           // "tail_pivot": the tail's dense LDL^T with diagonal pivoting (0: unpivoted, rounds 2 - 5)
    int tail_shard = 1;           // "tail_shard": world > 1, replicated solve: every rank applies 1 / world of the tail's rows, the K partial
                                  // results are all-reduced (0: every rank applies the whole tail)
    int l21_device = 1;           // "l21_device": hybrid y-solve allowed (L21 on the device beside the tail when the forest is too deep; 0: host, 2: whenever the sweeps stay on the host)
    int lead_debug = 0;           // "lead_debug": statistics of the leading elimination forest on stderr at init (developer aid)
    int lead_small_kb = 0;        // "lead_small_kb": LDS bound of the trees that share a workgroup in fours (lead_solve.h; 0 = chosen at build from 4 / 8 / 16)
    int lead_tops = -1;           // "lead_tops": dense tree tops (lead_solve.h): -1 = when the forest is too deep for the sweeps, 0 = never, L = always, cut at height L
    int debug_eig = 0;            // developer aid
  } sw;
  cuadmm_solver() {
    options_from_env(engine_option_table<cuadmm_solver>(), *this);
    plan.opt = PsdOptions::from_env();
  }
  int opt_tiny_sign = 1;       // option "tiny_sign": 0 never, 1 closed candidates, 2 always
  bool closed_candidate = false;
  int duo_cpu_eig_on_gpu = 0;
  int opt_hint = 1;            // option "psd_hint": 0 off, 1 one-wavefront kernels + mid-size blocks of the batched-GEMM path, 2 all, 3 one-wavefront kernels only
  LeadSolve lead;               // ... or, with a split factor, the leading sweeps on the device around the GPU tail (lead_solve.hip)
  int forest_trees = 0;
  DevBuf<int> f_tree_ptr, f_tree_cols, f_Li;
  DevBuf<long long> f_Lp;
  DevBuf<double> f_Lx, f_D, y_best_d;
  std::vector<double> y_full;
  cuadmm_aat* fac = nullptr;
  TailSolve tail;              // dense trailing triangle of L on the GPU (tail.k == 0: whole solve on the host)
  std::vector<int> perm, perm_inv;
  std::vector<double> normA;      // original order
  std::vector<double> normA_p, b_p, y_p, Rp_p, y_best_p;
  bool y_registered = false;   // y_p.data() page-locked with hipHostRegister (its storage is never reallocated)
  double norm_borg = 1, norm_Corg = 1, bscale = 1, Cscale = 1, objscale = 1;
  double sig = 1, errRp = 0, errRd = 0, maxfeas = 0, pobj = 0, dobj = 0, relgap = 0, feasratio = 0;
  int prim_win = 0, dual_win = 0;
  double ratioconst = 1, sigmax = 1e3, sigmin = 1e-3;
  double best_KKT = 0, sgs_KKT = 0;
  bool have_best = false;
  int eig_fail_total = 0;

  // info
  int info_iter_num = 0;
  std::vector<double> info[8];

  // device
  DevBuf<int> At_rp, At_ci, A_rp, A_ci;
  AtyLongRows At_long;         // svec rows of At with more than 128 entries
  SpmvLongRows A_long;         // rows of A much longer than the average (trace / all-ones constraints)
  DevBuf<double> At_v, A_v;
  DevBuf<double> X, S, C, Rd1, Xb, Xproj, y_d, out_d, partials, X_best, S_best;
  DevBuf<int> steps_d, hint_d;
  std::vector<int> steps_h;
  long long lpt_next = 3, lpt_iters = 0;       // longest-block-first reordering: next event, iterations so far
  PinnedBuf<int> steps_pin;                    // batched launches: step counts fetched behind one batch, sorted during the next
  bool lpt_steps_ready = false;
  // Where the kernels write [A*X | sums | A*(S-C)]: the device buffer out_d when it has to be all-reduced, otherwise the
  // pinned host buffer h_out itself through its device mapping -- the results cross PCIe as the kernels produce them and
  // fetch_out is a stream synchronisation without a copy.
  double* out_w = nullptr;
  bool out_mapped = false;
  PinnedBuf<double> h_out, h_y;
  double A_avg_nnz = 1;
  PsdPlan plan;

  // Safeguarded Anderson acceleration behind the iteration (option "accel" = memory; accel.h, DESIGN.md "Acceleration").  The state is
  // u = (X, sigma S); fbuf holds f_k = (X, S) as the last plain iteration left them (the next iteration's u unless a candidate is
  // taken, and what a rejected candidate falls back to), ubuf a candidate, gbuf g_k, the rings the last `cols` differences.
  struct Accel {
    int mem = 0;
    double safeguard = 2.0, reg = 1e-10;
    DevBuf<double> ring_dF, ring_dG, state[2], gbuf, partials, dots, fb_y, fb_out;
    struct { double* p = nullptr; } fbuf, ubuf;      // the two state buffers by role (they trade places when a candidate is accepted)
    PinnedBuf<double> h_dots;
    DevBuf<int> fb_hint;              // the sign schedule's warm start is part of what an iteration reads and writes (as in batch_copy)
    unsigned fb_nproj = 0;
    long long fb_iters_done = 0;
    std::vector<double> h_fb_out, h_fb_Rp, h_fb_y;
    long long hs = 0;                 // distance of the S half from the X half: L rounded up to an even number
    int cols = 0, head = 0;           // columns held, ring slot the next column goes to
    bool have_prev = false;           // fbuf / gbuf hold the previous pair (f, g) of the current map
    bool pending = false;             // the iteration under way started from a candidate
    double gnorm2_prev = 0;           // ||g_k||^2 of the iteration the pending candidate was formed behind
    double G[kAccelMaxMem][kAccelMaxMem] = {};   // Gram matrix of the dG columns, by ring slot
    double sc[8] = {};                // host scalars of f_k beside a pending candidate
    int sc_win[2] = {0, 0};
    long long taken = 0, accepted = 0, rejected = 0, restarts = 0;
    double ms = 0;
    DevEvent ev[4];
  } aa;
  bool accel_on() const { return aa.mem > 0 && L > 0; }
  void accel_clear() { aa.cols = 0; aa.head = 0; aa.have_prev = false; aa.pending = false; }
  int accel_begin_solve();
  int accel_step(int iter, int max_iter, double stop_tol, int switch_admm, double tau, bool sig_changed, bool next_sig_may_change);
  int accel_reject();                                   // accel_step's two arms behind a candidate's verdict: back to the fallback f_k,
  int accel_candidate(int cols_new, double gnorm2);     // or the next candidate from the columns held

  // Infeasibility detection behind the iteration (option "infeas_check" = period p; infeas.h, DESIGN.md "Infeasibility certificates").
  // Every p iterations the differences of y and X against the snapshot taken p iterations earlier are tested for the two certificates.
  // The projections, their two svec work vectors and b on the device are the auxiliary projector's (aux).
  struct Infeas {
    int period = 0;
    double tol = 1e-6;
    DevBuf<double> xprev, yprev, dy, adx, partials, stats_d;
    PinnedBuf<double> h_stats;
    std::vector<std::pair<long long, long long>> free_rng;   // svec ranges of the unconstrained blocks
    bool have_snap = false;
    // of the last solve
    long long checks = 0;
    double scalar = 0, eta = 0, radius = 0, ms = 0;
    std::vector<double> cert;         // the ray of a verdict, scaled space and internal order (y: m, X: L)
    double bytes() const { return 8.0 * (double)(xprev.n + yprev.n + dy.n + adx.n + partials.n + stats_d.n); }
  } inf;
  bool infeas_on() const { return inf.period > 0 && L > 0; }
  // how the last solve ended and behind which iteration (cuadmm_get_status; 3, 4: infeas_step, 5: lb_step)
  int solve_status = 0, solve_status_iter = 0;
  void infeas_reset() { inf.have_snap = false; solve_status = 0; solve_status_iter = 0; inf.checks = 0; inf.scalar = inf.eta = inf.radius = 0; inf.cert.clear(); }
  int infeas_begin_solve();
  int infeas_step(int iter, double stop_tol);

  // Certified lower bound from trace bounds (cuadmm_set_trace_bounds, cuadmm_lower_bound, option "gap_check" = period p; lower_bound.h,
  // DESIGN.md "Certified lower bound").  M = A'y - C (the iteration's kernel, into the auxiliary projector's input vector), P = P+(M) through
  // its plan, then one pass of per-block norms and a combine kernel: four doubles cross.
  struct Lb {
    int period = 0;
    double tol = 0;                    // 0: the solve's stop_tol
    std::vector<double> R;             // the caller's bounds, one per block (empty: none set)
    bool R_dirty = false;
    DevBuf<double> ybuf, R_d, pairs, cpart, dpart, out_d;
    PinnedBuf<double> h_out;
    // of the last solve with the option on
    long long checks = 0;
    int best_iter = 0, verdict_iter = 0;
    double best_lb = 0, last_lb = 0, last_g = 0, ms = 0;
    double bytes() const { return 8.0 * (double)(ybuf.n + R_d.n + pairs.n + cpart.n + dpart.n + out_d.n); }      // its own; the reports add btasks and aux
  } lb;
  bool gap_on() const { return lb.period > 0 && L > 0; }
  void lb_reset() { lb.checks = 0; lb.best_iter = lb.verdict_iter = 0; lb.best_lb = lb.last_lb = lb.last_g = 0; }
  int lb_prepare();
  int lb_eval(const double* y_scaled_d, double out6[6], float* ms);
  int lb_report(double out8[8], double* per_block);
  int lb_step(int iter, double stop_tol);

  AuxProj aux;                 // (report_plans.h)
  // What the reports on a point share besides it ("The front of the point reports"): y scaled and in the engine's order
  // (y_caller null: the resident one) into dst, max(m, 1) doubles; A'y - C into aux.in and the 256 slot sums of b'y.
  int stage_scaled_y(double* dst, const double* y_caller);
  int dual_slack(const double* y_scaled_d, double* by_part);

  BlockTasksDev btasks;        // (report_plans.h)

  // Evaluation of a point (cuadmm_evaluate; evaluate.h, DESIGN.md "Evaluation of a point").  The point in the engine's scaled space: xs, ss
  // (allocated when a vector is passed, or the resident one is in the caller's units; behind a solve the scaled iterate is read where it
  // lies) and cons, which holds y and then A X.  px = P+(X); P+(S) and A'y - C go to the auxiliary projector's two vectors.  normA: the
  // column norms where the engine keeps them on the host only (as AuxProj::bcopy for b).  Nothing here is read by the iteration.
  struct Ev {
    DevBuf<double> xs, ss, px, cons, normA, sums, cpart, part, out_d;
    PinnedBuf<double> h_out;
    long long calls = 0;
    double ms = 0;
    double bytes() const { return 8.0 * (double)(xs.n + ss.n + px.n + cons.n + normA.n + sums.n + cpart.n + part.n + out_d.n); }      // its own
  } ev;
  int ev_prepare();
  int ev_point(const double* host, const DevBuf<double>& resident, double inv_scale, DevBuf<double>& own, const double** out);
  int ev_run(const double* xs, const double* ss, double out16[16], double* per_block);

  LmPlan lm;                   // (report_plans.h)
  int lm_prepare(int which);
  int lm_run(int which, int steps, double out8[8], double* per_block);

  LrPlan lr;                   // (report_plans.h)
  int lr_prepare(int rmax);
  int lr_run(int which, double tol, double out8[8], double* per_block, double* L_out, int* piv_out);

  FactorLayoutDev fl;          // (report_plans.h): the callers' factor layout of the five calls below, prepared by each for its rmax
  LoPlan lo;                   // (report_plans.h): cuadmm_set_lowrank

  BmPlan bm;                   // (report_plans.h): cuadmm_block_multiply
  int bm_prepare(int which, int rmax);
  int bm_run(int which, const double* V, const int* ranks, double* W_out, double out8[8], double* per_block);

  LgPlan lg;                   // (report_plans.h): cuadmm_lowrank_grad
  int lg_prepare(int rmax);
  int lg_run(const double* Lf, const int* ranks, double sigma, double* G_out, double* r_out, double* Shat_out, double out8[8], double* per_block);

  LlPlan ll;                   // (report_plans.h): cuadmm_lowrank_line
  int ll_prepare(int rmax);
  int ll_run(const double* Lf, const double* Df, const int* ranks, double sigma, double t_max, double coef5[5], double* r_out, double* p_out, double* q_out,
             double out8[8], double* per_block);
  int lg_enqueue(const double* Lx, double sigma, bool block_terms);      // the chains of lg_run / ll_run on resident buffers, nothing fetched
  int ll_enqueue();
  int ll_coef(double sigma, double ux, double c[5], double sm[kLlParts], const double** sums);

  RfPlan rf;                   // (report_plans.h): cuadmm_lowrank_refine
  int rf_prepare(int rmax);
  int rf_run(const double* Lf, const int* ranks, double sigma, int steps, double t_max, double gtol, double* L_out, double* trace, double out8[8], double* r_out);

  // profiling
  DevEvent ev0[K_NUM][2], ev1[K_NUM][2];
  int ev_used[K_NUM] = {0};
  double prof_count[K_NUM] = {0}, prof_ms[K_NUM] = {0}, prof_bytes[K_NUM] = {0};

  ~cuadmm_solver() {
    if (y_registered) { hipError_t e = hipHostUnregister(y_p.data()); (void)e; }
    if (fac) cuadmm_aat_free(fac);
    if (st) { hipError_t e = hipStreamDestroy(st); (void)e; }
    if (rccl_comm && g_rccl.CommDestroy) { g_rccl.CommDestroy(rccl_comm); rccl_comm = nullptr; }
  }

  bool prof_on(int k) const { return profile == 1 || (profile == 2 && k == K_PSD); }
  void prof_begin(int k) {
    if (!prof_on(k) || ev_used[k] >= 2) return;
    hipError_t e = hipEventRecord(ev0[k][ev_used[k]], st); (void)e;
  }
  void prof_end(int k, double bytes) {
    if (!prof_on(k) || ev_used[k] >= 2) return;
    hipError_t e = hipEventRecord(ev1[k][ev_used[k]], st); (void)e;
    ev_used[k]++;
    prof_bytes[k] = bytes;
  }
  void prof_collect() {  // call after a stream synchronize
    if (!profile) return;
    for (int k = 0; k < K_NUM; ++k) {
      for (int j = 0; j < ev_used[k]; ++j) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev0[k][j], ev1[k][j]) == hipSuccess) { prof_ms[k] += ms; prof_count[k] += 1; }   // (a sample only where the read succeeds)
      }
      ev_used[k] = 0;
    }
  }
  void prof_host(int k, double seconds) {
    if (profile != 1) return;
    prof_ms[k] += seconds * 1e3; prof_count[k] += 1;
  }

  int do_allreduce(double* buf, size_t count) {
    if (world <= 1 && !force_comm) return CUADMM_OK;
    return comm_allreduce(buf, count);
  }
  int comm_allreduce(double* buf, size_t count);      // all-reduce over the communicator (the sharding world, or comm_world in owned-constraints mode)
  int allreduce_scalars(double* v, int n);            // owned-constraints mode: v[0..n) <- sum over ranks (host values through a small device buffer; blocks)
  // y_p = (P(AA^T+eps I)P^T)^-1 rhs_p; in_fused_step: the projection launch that follows solves for y itself (closed blocks)
  int host_solve(bool in_fused_step = false);
  int upload_y(bool force = false);                   // y_p -> y_d (nothing to do with the y-solve on the device, unless forced)
  // D2H of out_d[first, first+count) after the optional all-reduce; blocks until it has landed.  solve_next: engine_iter.hip
  bool y_early = false;           // y_d already holds the y-solve of the coming iteration
  DevEvent ev_early;
  int fetch_out(size_t first, size_t count, bool solve_next = false);
  int launch_aty(bool write_xb);
  // after_fused: the local rows were written by the fused projection kernels of this step -- only the other rows are left
  int launch_spmv(bool doX, bool doS, bool after_fused = false);
  int launch_project();
  int launch_fused_step(int mode, double tau, int iters = 1);      // Step 2 of a fused iteration; iters > 1: a batch
  int launch_post_mode(int mode, double tau);
  // --- several iterations per launch ---------------------------------------------------------------------------------
  bool can_batch() const;
  bool can_batch_local() const;
  int batch_agree();            // the ranks take the batching decision together, once per solve
  int batch_alloc();
  int batch_copy(bool save);    // checkpoint of everything an iteration reads and writes: X, S, y, [A X | sums | A (S - C)]
  int batch_rollback(int keep); // back to the checkpoint and forward again by the `keep` iterations the host schedule accepted
  // X, S, y back in the caller's units (solver.cu:814-816); a no-op unless a solve left them scaled
  int materialise();
  int sync_y_host();
  int reset_solve_state(double t_begin);

  // bscale from nb2 = sum (b_i / normA_i)^2 and b_p from bfull = b / normA (this rank's constraints, the caller's order): solver.cu:169-191
  void set_scaled_b(const std::vector<double>& bfull, double nb2) {
    bscale = 1 + std::sqrt(nb2);
    const double ibs = 1 / bscale;             // *_div_scalar multiply by 1/s (dense_scalar.cu:77-81)
    for (int pidx = 0; pidx < m; ++pidx) b_p[pidx] = bfull[perm[pidx]] * ibs;
  }
  // Rp = b - A X from the fetched A X (host y-solve; with the solve on the device Rp never exists on the host)
  void refresh_Rp() {
    for (int i = 0; i < m && !dev_solve; ++i) Rp_p[i] = -h_out.p[i] + b_p[i];
  }
  // the scalars of the stopping test (solver.cu:195-228, 764-799) from nr = ||normA Rp bscale||^2, b'y and the two sums behind A X in h_out
  void set_residual_scalars(double nr, double bty) {
    errRp = std::sqrt(nr) / norm_borg;
    errRd = std::sqrt(h_out.p[(size_t)m]) * Cscale / norm_Corg;
    maxfeas = std::max(errRp, errRd);
    pobj = h_out.p[(size_t)m + 1] * objscale;
    dobj = bty * objscale;
    relgap = std::fabs(pobj - dobj) / (1 + std::fabs(pobj) + std::fabs(dobj));
  }
};

using Solver = cuadmm_solver;

// `in_group_call` marks the calls an in-process group (duo_group.hip) makes on its own ranks, rank 0 -- the leader itself -- included
template <class F>
int as_group_rank(cuadmm_solver* q, F&& call) {
  q->in_group_call = true;
  const int rc = call(q);
  q->in_group_call = false;
  return rc;
}
// the leader forwards an entry point: every rank runs `call`, ranks >= 1 on their own host threads
template <class F>
int group_forward(cuadmm_solver* s, F&& call) {
  DeviceGuard keep_device;                  // the ranks' devices are made current on this thread: leave the caller's as it was
  return duo_group_run(s->group, [&](cuadmm_solver* q, int) { return as_group_rank(q, call); });
}

namespace cuadmm {
// SDPSolver::init, in stages (engine.hip).  InitIn: the caller's arrays (solver.h:208-223); InitCtx: what one stage leaves for the next.
struct InitIn {
  int vec_len, con_num, At_nnz, b_nnz, C_nnz, mat_num;
  const int *At_cp, *At_ri, *b_idx, *C_idx, *blk;
  const double *At_vx, *b_vals, *C_vals, *X0, *y0, *S0;
  double sig;
};
struct InitCtx {
  std::vector<double> vals;      // A^T values with the columns normalised (get_normA)
  std::vector<int> rp, rci;      // A^T in CSR over the svec rows: row pointers, constraint of every entry
  std::vector<double> rv;
};

// init's helpers and stages that cuadmm_update_bC / cuadmm_update_A (engine_update.hip) run again; defined in engine.hip
double cons_norm(const double* v, int lo, int hi);
double sum_sq(const double* v, int n);
int check_sparse_idx(const char* who, const char* what, const int* idx, int nnz, long long n);
double sum_scaled_sq(const int* idx, const double* val, int nnz, const double* norm);
double scaled_b(const int* idx, const double* val, int nnz, const int* g2l, const std::vector<double>& normA, std::vector<double>& full);
int init_normalise(Solver* s, const InitIn& in, InitCtx& c);
int tail_probe(Solver* s, const int64_t* srp, const int* sci, const double* sv, int tk, bool& tail_ok);
int init_solve_plan(Solver* s, const InitIn& in, InitCtx& c);
int init_closed(Solver* s, const InitIn& in, InitCtx& c);
int init_residuals(Solver* s, bool y_resident);

inline const double* AuxProj::b_dev(const cuadmm_solver& s) const { return s.b_d.p ? s.b_d.p : bcopy.p; }
}  // namespace cuadmm
