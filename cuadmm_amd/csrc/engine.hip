// The SDP-ADMM iteration engine: MI355X-native replacement of SDPSolver::init / ::solve
// (reference src/solver.cu:27-342 and :355-823).
//
// Data layout (all fp64, resident in HBM for the whole solve):
//   X, S, C, Rd1, Xb, Xproj : svec vectors of this rank's contiguous block range
//   At_csr  : rows = local svec slots, columns = constraints in the factor's PERMUTED order
//   A_csr   : rows = constraints in permuted order, columns = local svec slots
//   out     : [A*X (m) | sum Rd^2 | sum C.X | A*(S-C) (m)]  -> one D2H per (half-)iteration
// The constraint-space vectors (y, b, normA; length m) are kept in the PERMUTED order of the LDL^T factor of P(AA^T + eps I)P^T, so the
// reference's two scatter kernels per solve (perform_permutation, solver.cu:487,500) disappear: the permutation is folded into the
// matrices.  The factor is computed once on the host; the solve runs on the device whenever the plan allows it (every shipped input):
// level sweeps over the shallow rest of the elimination forest, packed inverses of the tree tops, and the dense tail W = inv(L22) applied
// in one pass (lead_solve.hip, tail_solve.hip; DESIGN.md sections 3 - 4).  y then never leaves the device: the host fetches the four
// scalars of the stopping test per iteration through a mapped pinned buffer.  With the solve on the host (option host_solve, or a probe
// that rejects the explicit inverse) the traffic per iteration is m doubles up (y), 2m+2 doubles down (ADMM phase).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <iostream>
#include <numeric>

#include "device_util.h"
#include "psd_plan.h"
#include "tail_solve.h"
#include "lead_solve.h"
#include "vec_kernels.h"
#include "duo_group.h"
#include "accel.h"
#include "infeas.h"
#include "lower_bound.h"
#include "evaluate.h"
#include "lambda_min.h"
#include "lowrank.h"

using namespace cuadmm;

namespace {

double wall_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  int alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return CUADMM_OK;
    CUADMM_HIP_TRY(hipMalloc(&p, sizeof(T) * count));
    return CUADMM_OK;
  }
  int upload(const T* h, size_t count) {
    if (count == 0) return CUADMM_OK;
    return staged_h2d(p, h, sizeof(T) * count);   // never hipMemcpy on caller / vector memory (staging.hip)
  }
  int from(const std::vector<T>& h, size_t pad = 0) {   // pad: extra (zeroed) elements behind the data
    int rc = alloc(h.size() + pad);
    if (rc) return rc;
    n = h.size();
    if (pad) CUADMM_HIP_TRY(hipMemset(p + h.size(), 0, sizeof(T) * pad));
    return upload(h.data(), h.size());
  }
  void release() {
    if (p) { hipError_t e = hipFree(p); (void)e; }
    p = nullptr; n = 0;
  }
  ~DevBuf() { release(); }
};

template <class T>
struct PinnedBuf {
  T* p = nullptr;
  size_t n = 0;
  int alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return CUADMM_OK;
    CUADMM_HIP_TRY(hipHostMalloc(&p, sizeof(T) * count, hipHostMallocDefault));
    return CUADMM_OK;
  }
  void release() {
    if (p) { hipError_t e = hipHostFree(p); (void)e; }
    p = nullptr; n = 0;
  }
  ~PinnedBuf() { release(); }
};

// Host loops over the m constraints: serial below kHostParMin, else kHostChunks fixed index ranges on the host pool
// (aat_ldlt.cpp).  Sums are formed per range and combined in range order: reproducible for any thread count.
constexpr int kHostParMin = 20000, kHostChunks = 32;
constexpr size_t kSvecPad = 64 * 40;       // >= 64 * U * batches of every tile geometry (psd_sign_closed.h)
template <class F>
static void host_ranges(int m, F&& body) {   // body(chunk, lo, hi)
  if (m < kHostParMin) { body(0, 0, m); return; }
  struct Ctx { F* f; int m; } ctx{&body, m};
  cuadmm_host_parallel_for(kHostChunks, [](int c, void* p) {
    Ctx* x = static_cast<Ctx*>(p);
    const long long lo = (long long)x->m * c / kHostChunks, hi = (long long)x->m * (c + 1) / kHostChunks;
    (*x->f)(c, (int)lo, (int)hi);
  }, &ctx);
}

// milliseconds between two recorded events; 0, with the runtime's error cleared, where it cannot tell
static float event_ms(hipEvent_t a, hipEvent_t b) {
  float t = 0;
  if (hipEventElapsedTime(&t, a, b) != hipSuccess) { t = 0; (void)hipGetLastError(); }
  return t;
}

enum KClass { K_ATY = 0, K_PSD = 1, K_POST = 2, K_SPMV = 3, K_COPY = 4, K_HOST = 5, K_COMM = 6, K_TAIL = 7, K_NUM = CUADMM_NUM_KCLASS };

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
RcclApi g_rccl;

}  // namespace

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
  // calls the group makes on its own ranks.  option_log: every cuadmm_set_option so far (replayed on the group's children).
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
    hipEvent_t ev[4] = {};
    double pass_ms[2] = {0, 0}, pass_bytes[2] = {0, 0};
    ~UpdateA() { for (auto& e : ev) if (e) { hipError_t r = hipEventDestroy(e); (void)r; } }
  } upa;
  bool factor_bad = false;
  // Behavioural switches (cuadmm_set_option, before init).  The environment variables of round 1 / 2 only give the DEFAULTS, read
  // once per solver in its constructor: two solvers in a process can choose differently, and tests reach every variant.
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
    auto env = [](const char* n, int d) { const char* e = getenv(n); return e ? atoi(e) : d; };
    sw.fuse = env("CUADMM_FUSE", 1); sw.fuse_rows = env("CUADMM_FUSE_ROWS", 1); sw.fuse_solve = env("CUADMM_FUSE_SOLVE", -1);
    sw.host_solve = env("CUADMM_HOST_SOLVE", 0); sw.tail_k = env("CUADMM_TAIL_K", -1);
    sw.local_constraints = env("CUADMM_NO_LOCAL_CONSTRAINTS", 0) ? 0 : 1;
    sw.mapped_out = env("CUADMM_NO_MAPPED_OUT", 0) ? 0 : 1;
    sw.host_scalars = env("CUADMM_HOST_SCALARS", 0);
    opt_hint = env("CUADMM_PSD_HINT", 1);
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
    hipEvent_t ev[4] = {};
    ~Accel() { for (auto& e : ev) if (e) { hipError_t r = hipEventDestroy(e); (void)r; } }
  } aa;
  bool accel_on() const { return aa.mem > 0 && L > 0; }
  void accel_clear() { aa.cols = 0; aa.head = 0; aa.have_prev = false; aa.pending = false; }
  int accel_begin_solve();
  int accel_step(int iter, int max_iter, double stop_tol, int switch_admm, double tau, bool sig_changed, bool next_sig_may_change);

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

  // The auxiliary projector of the infeasibility check and the lower bound ("Infeasibility certificates"): a plan beside the
  // iteration's, an svec-length input and output vector, b on the device where the engine keeps none there, a pair of events.  The two
  // users never run inside one another and the plan carries no result from one projection to the next, so one object serves both.
  struct AuxProj {
    PsdPlan* plan = nullptr;           // built at the first projection: the solver's psd_* options, the full projection
    DevBuf<double> in, out, bcopy;
    double plan_bytes = 0;
    hipEvent_t ev[2] = {};
    bool projected = false;            // inside the open bracket
    int ensure(cuadmm_solver& s);      // vectors and events on first use; b, which may have changed, on every call
    const double* b_dev(const cuadmm_solver& s) const { return s.b_d.p ? s.b_d.p : bcopy.p; }
    int project(cuadmm_solver& s, const double* from, double* to);
    bool failed(hipStream_t st) const { return plan && plan->fail_count(st) > 0; }
    // The bracket around one user's work on the stream.  end: the stream is drained; *ms between the two events; *bad: a projection
    // inside the bracket was made and the plan's (cumulative) failure count is not zero -- the user words its own CUADMM_ERR_EIG
    // (null for a user that projects nothing).
    int begin(hipStream_t st) { projected = false; CUADMM_HIP_TRY(hipEventRecord(ev[0], st)); return CUADMM_OK; }
    int end(hipStream_t st, float* ms, bool* bad) {
      CUADMM_HIP_TRY(hipEventRecord(ev[1], st));
      CUADMM_HIP_TRY(hipStreamSynchronize(st));
      *ms = event_ms(ev[0], ev[1]);
      if (bad) *bad = projected && failed(st);
      return CUADMM_OK;
    }
    double bytes() const { return 8.0 * (double)(in.n + out.n + bcopy.n) + plan_bytes; }
    ~AuxProj() { for (auto& e : ev) if (e) { hipError_t r = hipEventDestroy(e); (void)r; } delete plan; }
  } aux;
  // What the reports on a point share besides it ("The front of the point reports"): y scaled and in the engine's order
  // (y_caller null: the resident one) into dst, max(m, 1) doubles; A'y - C into aux.in and the 256 slot sums of b'y.
  int stage_scaled_y(double* dst, const double* y_caller);
  int dual_slack(const double* y_scaled_d, double* by_part);

  // The per-block task lists of block_reduce.h on the device, for the lower bound and the evaluation: built from blk_local by whichever
  // of lb_prepare / ev_prepare runs first.  blk_local never changes after init, so cuadmm_update_A / cuadmm_update_bC leave them alone.
  // Each of the two reports these bytes with its own, as it does the auxiliary projector's.
  struct BlockTasksDev {
    DevBuf<long long> off, len;
    DevBuf<int> blk, wave, chunk, large;
    int nwave = 0, nchunk = 0, nlarge = 0;
    bool built = false;
    int build(const int* blk_h, int nb, const int64_t* off_h /* null: consecutive */) {
      std::vector<long long> o((size_t)nb), l((size_t)nb);
      long long next = 0;
      for (int k = 0; k < nb; ++k) { l[k] = blk_svec_len(blk_h[k]); o[k] = off_h ? (long long)off_h[k] : next; next += l[k]; }
      BlockTasks t;
      int rc;
      if ((rc = build_block_tasks(nb, l.data(), &t)) || (rc = off.from(o)) || (rc = len.from(l)) || (rc = blk.from(std::vector<int>(blk_h, blk_h + nb))) ||
          (rc = wave.from(t.wave)) || (rc = chunk.from(t.chunk)) || (rc = large.from(t.large)))
        return rc;
      nwave = t.nwave(); nchunk = t.nchunk(); nlarge = t.nlarge();
      built = true;
      return CUADMM_OK;
    }
    BlockTasksView view() const { return {off.p, len.p, blk.p, wave.p, chunk.p, large.p, nwave, nchunk, nlarge}; }
    double bytes() const { return 8.0 * (double)(off.n + len.n) + 4.0 * (double)(blk.n + wave.n + chunk.n + large.n); }
  } btasks;

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

  // Certified lambda_min per block (cuadmm_lambda_min, cuadmm_op_block_lambda_min; lambda_min.h, DESIGN.md "Certified lambda_min"): the
  // size classes' block lists on the device, the global scratch of the blocks beyond the LDS (only where there are such), the results.
  // The offsets and sizes per block are the task lists' (btasks).  Nothing here is read by the iteration.
  struct LmPlan {
    LmClass cls[kLmClasses];
    DevBuf<int> list[kLmClasses];
    DevBuf<long long> work_off;
    DevBuf<double> work, out, ybuf, dpart;
    PinnedBuf<double> h_out;
    int nb = 0;
    long long calls = 0;
    int build(const int* blk_h, int nblk) {
      long long w = 0;
      int rc = lm_build_classes(nblk, blk_h, cls, &w);
      if (rc) return rc;
      for (int q = 0; q < kLmClasses; ++q)
        if ((rc = list[q].from(cls[q].blocks))) return rc;
      if ((rc = work_off.from(cls[kLmClasses - 2].work)) || (rc = work.alloc((size_t)w)) || (rc = h_out.alloc(kLmOut * (size_t)nblk + kBrSlots))) return rc;
      nb = nblk;
      return out.alloc(kLmOut * (size_t)nblk);      // last: marks the set as complete
    }
    // out (device) <- the four numbers per block of sign * v; one launch per class that has blocks
    int run(const double* v, double sign, const long long* off_d, const int* blk_d, int steps, hipStream_t st) {
      int rc;
      for (int q = 0; q < kLmClasses; ++q)
        if ((rc = launch_lambda_min(q, (int)cls[q].blocks.size(), cls[q].nmax, list[q].p, v, sign, off_d, blk_d, steps, work.p, work_off.p, out.p, st))) return rc;
      return CUADMM_OK;
    }
    double bytes() const {
      double b = 8.0 * (double)(work_off.n + work.n + out.n + ybuf.n + dpart.n);
      for (const auto& l : list) b += 4.0 * (double)l.n;
      return b;
    }
  } lm;
  int lm_prepare(int which);
  int lm_run(int which, int steps, double out8[8], double* per_block);

  // Rank and low-rank factor per block (cuadmm_lowrank, cuadmm_op_block_lowrank; lowrank.h, DESIGN.md "Low-rank factors"): the size
  // classes' block lists, the offsets of the blocks' factors and pivots for the rmax of the last call, the factor, pivot and result
  // buffers (they grow with rmax and are kept), a pair of events.  The offsets and sizes per block are the task lists' (btasks).  Nothing
  // here is read by the iteration.
  struct LrPlan {
    LrClass cls[kLrClasses];
    DevBuf<int> list[kLrClasses], piv;
    DevBuf<long long> loff_d, poff_d;
    DevBuf<double> Lbuf, out;
    std::vector<long long> loff, poff;      // of rmax_now, nb + 1 entries each
    int nb = 0, rmax_now = 0;
    hipEvent_t ev[2] = {};
    long long calls = 0;
    int prepare(const int* blk_h, int nblk, int rmax) {
      if (out.p && rmax == rmax_now) return CUADMM_OK;
      int rc = lr_build_classes(nblk, blk_h, rmax, cls, &loff, &poff);
      if (rc) return rc;
      const bool first = !out.p;
      if (first) {
        for (int q = 0; q < kLrClasses; ++q)
          if ((rc = list[q].from(cls[q].blocks))) return rc;
        if ((rc = loff_d.alloc((size_t)nblk + 1)) || (rc = poff_d.alloc((size_t)nblk + 1))) return rc;
        for (auto& e : ev) CUADMM_HIP_TRY(hipEventCreate(&e));
      }
      rmax_now = 0;                           // (until the offsets on the device are this rmax's)
      if ((rc = loff_d.upload(loff.data(), loff.size())) || (rc = poff_d.upload(poff.data(), poff.size()))) return rc;
      if (Lbuf.n < (size_t)loff.back() + 1 && (rc = Lbuf.alloc((size_t)loff.back() + 1))) return rc;      // (+ 1: never empty)
      if (piv.n < (size_t)poff.back() + 1 && (rc = piv.alloc((size_t)poff.back() + 1))) return rc;
      nb = nblk;
      rmax_now = rmax;
      return first ? out.alloc(kLrOut * (size_t)nblk) : CUADMM_OK;      // last: marks the set as complete
    }
    // out, Lbuf, piv (device) <- the kernel's results on sign * v; one launch per class that has blocks
    int run(const double* v, double sign, const long long* off_d, const int* blk_d, double tol, hipStream_t st) {
      int rc;
      for (int q = 0; q < kLrClasses; ++q)
        if ((rc = launch_lowrank(q, (int)cls[q].blocks.size(), cls[q].nmax, list[q].p, v, sign, off_d, blk_d, tol, rmax_now, loff_d.p, poff_d.p, Lbuf.p, piv.p,
                                 out.p, st)))
          return rc;
      return CUADMM_OK;
    }
    // The results behind a drained stream, on the host and in the units `unit` times the vector's: per_block (kLrOut nb, not null); L_out
    // (may be null): loff.back() doubles; piv_out (may be null): as many ints, block k's min(n_k, rmax) pivots at loff[k], -1 elsewhere.
    int fetch(double unit, double* per_block, double* L_out, int* piv_out) {
      int rc;
      if (nb > 0 && (rc = staged_d2h(per_block, out.p, sizeof(double) * kLrOut * (size_t)nb))) return rc;
      for (int k = 0; k < nb; ++k)
        for (int q = 1; q <= 3; ++q) per_block[kLrOut * (size_t)k + q] *= unit;
      const size_t count = (size_t)loff.back();
      if (L_out && count > 0) {
        if ((rc = staged_d2h(L_out, Lbuf.p, sizeof(double) * count))) return rc;
        const double root = std::sqrt(unit);
        for (size_t e = 0; unit != 1.0 && e < count; ++e) L_out[e] *= root;
      }
      if (piv_out && count > 0) {
        std::vector<int> h((size_t)poff.back() + 1);
        if ((rc = staged_d2h(h.data(), piv.p, sizeof(int) * (size_t)poff.back()))) return rc;
        std::fill(piv_out, piv_out + count, -1);
        for (int k = 0; k < nb; ++k) std::copy(h.begin() + poff[k], h.begin() + poff[k + 1], piv_out + loff[k]);
      }
      return CUADMM_OK;
    }
    double bytes() const {
      double b = 8.0 * (double)(loff_d.n + poff_d.n + Lbuf.n + out.n) + 4.0 * (double)piv.n;
      for (const auto& l : list) b += 4.0 * (double)l.n;
      return b;
    }
    ~LrPlan() { for (auto& e : ev) if (e) { hipError_t r = hipEventDestroy(e); (void)r; } }
  } lr;
  int lr_prepare(int rmax);
  int lr_run(int which, double tol, double out8[8], double* per_block, double* L_out, int* piv_out);

  // profiling
  hipEvent_t ev0[K_NUM][2] = {}, ev1[K_NUM][2] = {};
  int ev_used[K_NUM] = {0};
  double prof_count[K_NUM] = {0}, prof_ms[K_NUM] = {0}, prof_bytes[K_NUM] = {0};

  ~cuadmm_solver() {
    if (y_registered) { hipError_t e = hipHostUnregister(y_p.data()); (void)e; }
    if (fac) cuadmm_aat_free(fac);
    for (int k = 0; k < K_NUM; ++k)
      for (int j = 0; j < 2; ++j) {
        if (ev0[k][j]) { hipError_t e = hipEventDestroy(ev0[k][j]); (void)e; }
        if (ev1[k][j]) { hipError_t e = hipEventDestroy(ev1[k][j]); (void)e; }
      }
    if (ev_early) { hipError_t e = hipEventDestroy(ev_early); (void)e; }
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
  // all-reduce over the communicator (the sharding world, or comm_world in owned-constraints mode)
  int comm_allreduce(double* buf, size_t count) {
    prof_begin(K_COMM);
    int rc = 0;
    if (allreduce) {
      rc = allreduce(allreduce_user, buf, count, (void*)st);
    } else if (rccl_comm) {
      rc = g_rccl.AllReduce(buf, buf, count, /*ncclFloat64*/ 8, /*ncclSum*/ 0, rccl_comm, st);
    } else {
      set_error("world=%d but no all-reduce hook installed (cuadmm_set_allreduce / cuadmm_use_rccl)", local_mode ? comm_world : world);
      return CUADMM_ERR_COMM;
    }
    prof_end(K_COMM, (double)count * 8);
    if (rc) { set_error("all-reduce hook failed with code %d", rc); return CUADMM_ERR_COMM; }
    return CUADMM_OK;
  }

  // owned-constraints mode: v[0..n) <- sum over ranks (host values through a small device buffer; blocks)
  int allreduce_scalars(double* v, int n) {
    if (!local_mode || comm_world <= 1) return CUADMM_OK;
    // through the page-locked h_scal: the runtime must never register stack or caller memory (staging.hip)
    for (int q = 0; q < n; ++q) h_scal.p[q] = v[q];
    CUADMM_HIP_TRY(hipMemcpyAsync(scal_d.p, h_scal.p, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    int rc = comm_allreduce(scal_d.p, (size_t)n);
    if (rc) return rc;
    CUADMM_HIP_TRY(hipMemcpyAsync(h_scal.p, scal_d.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    CUADMM_HIP_TRY(hipStreamSynchronize(st));
    for (int q = 0; q < n; ++q) v[q] = h_scal.p[q];
    return CUADMM_OK;
  }

  // in_fused_step: the projection launch that follows solves for y itself (closed blocks)
  int host_solve(bool in_fused_step = false) {  // y_p = (P(AA^T+eps I)P^T)^-1 rhs_p
    double t0 = wall_s();
    const double isig = 1 / sig;
    if (in_fused_step && closed.active) return CUADMM_OK;
    if (dev_solve) {   // everything it needs is in HBM (out_d: [A X | sums | A(S-C)]); y_d is the result
      prof_begin(K_TAIL);
      int rc = lead.ready ? lead.solve(out_d.p, out_d.p + (size_t)m + 2, b_d.p, isig, y_d.p, tail, st) : launch_forest_solve(forest_trees, f_tree_ptr.p, f_tree_cols.p, f_Lp.p, f_Li.p, f_Lx.p, f_D.p, out_d.p, out_d.p + (size_t)m + 2,
                                   b_d.p, isig, y_d.p, st);
      prof_end(K_TAIL, tail.k > 0 ? tail.shard_bytes : 0.0);     // bytes of inv(L22) this rank read (1 / world of 4 K^2 when the tail is sharded)
      return rc;
    }
    // the right-hand side is formed in y_p from the pinned result buffer (A(S-C) lives at h_out[m+2..) since the last
    // fetch) and solved in place: no copies of m-vectors on the critical path between two GPU phases
    const double* asmc = h_out.p + (size_t)m + 2;
    host_ranges(m, [&](int, int lo, int hi) {
      for (int i = lo; i < hi; ++i) y_p[i] = -asmc[i] + isig * Rp_p[i];   // solver.cu:478-482
    });
    int rc;
    if (tail.k == 0) {
      rc = cuadmm_aat_solve_permuted(fac, y_p.data(), y_p.data());     // solver.cu:494
    } else {   // sparse leading columns here, dense trailing triangle on the GPU
      // hybrid (lead_solve.h): L21 lives on the device with the tail, the host sweeps L11 only
      rc = lead.hybrid ? cuadmm_aat_solve_leading_forward11(fac, tail.k, y_p.data()) : cuadmm_aat_solve_leading_forward(fac, tail.k, y_p.data());
      double t1 = wall_s();
      if (!rc) rc = lead.hybrid ? lead.apply_l21(y_p.data(), y_registered, tail, st) : tail.solve(y_p.data() + (m - tail.k), st);
      double t2 = wall_s();
      prof_host(K_TAIL, t2 - t1);
      t0 += t2 - t1;
      if (!rc) rc = lead.hybrid ? cuadmm_aat_solve_leading_backward11(fac, tail.k, y_p.data(), lead.h_w) : cuadmm_aat_solve_leading_backward(fac, tail.k, y_p.data());
    }
    prof_host(K_HOST, wall_s() - t0);
    return rc;
  }

  int upload_y(bool force = false) {
    if (dev_solve && !force) return CUADMM_OK;     // y is produced on the device
    prof_begin(K_COPY);
    // y_p is registered (page-locked) at init: the copy engine reads it directly; it is not written again before the
    // next fetch_out has synchronised the stream
    const double* src = y_p.data();
    if (!y_registered) { std::memcpy(h_y.p, y_p.data(), sizeof(double) * (size_t)m); src = h_y.p; }
    CUADMM_HIP_TRY(hipMemcpyAsync(y_d.p, src, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, st));
    prof_end(K_COPY, (double)m * 8);
    return CUADMM_OK;
  }

  // D2H of out_d[first, first+count) after the optional all-reduce; blocks until it has landed.
  // solve_next (round 5): the y-solve of the NEXT iteration is enqueued behind this iteration's last kernel BEFORE the host waits --
  // and the host then waits for an event recorded in front of it, not for the stream.  The reference solves for y at the top of every
  // pass through the loop, the breaking one included (solver.cu:478-500 precede the break), so that solve is never speculative; its only
  // host input is sigma, which the caller knows will not change in this iteration's step 5.  The GPU runs the solve (0.2 - 0.4 ms on the
  // moment relaxations) while the host goes through the stopping test and enqueues the rest of the next iteration: the idle gap at
  // the iteration boundary (kernel trace: the largest one of a latency-bound iteration) is gone.
  bool y_early = false;           // y_d already holds the y-solve of the coming iteration
  hipEvent_t ev_early = nullptr;
  int fetch_out(size_t first, size_t count, bool solve_next = false) {
    if (!out_mapped) {
      int rc = do_allreduce(out_d.p + first, count);
      if (rc) return rc;
      if ((dev_scalars || dev_solve) && first == 0) {     // [||Rp||^2, b.y, sum Rd^2, <C,X>] (of this rank -> sum over ranks), on the stream
        // without a collective in between the final stage writes the four scalars straight into the pinned host buffer
        // through its device mapping: the fetch is then a stream synchronisation without a copy command
        double* dst = (!dev_scalars && h_scal_dev) ? h_scal_dev : scal_d.p;
        if (stats_fused) stats_fused = false;               // formed by launch_reduce_quads in this iteration's fused step
        else if ((rc = launch_rp_stats(m, out_d.p, b_d.p, normA_d.p, y_d.p, bscale, out_d.p + (size_t)m, scal_d.p + 8, dst, st))) return rc;
        if (dev_scalars) {
          if ((rc = comm_allreduce(scal_d.p, 4))) return rc;
        }
        if (dst == scal_d.p) CUADMM_HIP_TRY(hipMemcpyAsync(h_scal.p, scal_d.p, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
      }
      if (dev_solve) {
        if (first != 0) return CUADMM_OK;                 // sGS half step: A(S-C) is consumed on the device, nothing to wait for
      } else {
        CUADMM_HIP_TRY(hipMemcpyAsync(h_out.p + first, out_d.p + first, sizeof(double) * count, hipMemcpyDeviceToHost, st));
      }
    }
    // (measured and rejected, round 5: a one-thread kernel storing a sequence number into a mapped pinned word with the host spinning on
    // it instead of this call -- c5 2 494 -> 2 476, c1 1 290 -> 1 274 iters/s: the runtime's wait already spins, the extra launch costs)
    if (solve_next && dev_solve && !out_mapped && st != nullptr) {
      // system-scope release: the host reads the pinned h_scal / h_out behind this wait (the stream synchronisation it replaces was one)
      if (!ev_early) CUADMM_HIP_TRY(hipEventCreateWithFlags(&ev_early, hipEventDisableTiming | hipEventReleaseToSystem));
      CUADMM_HIP_TRY(hipEventRecord(ev_early, st));
      { int rc = host_solve(); if (rc) { (void)hipStreamSynchronize(st); return rc; } }     // nothing of this iteration stays in flight behind an error
      y_early = true;
      CUADMM_HIP_TRY(hipEventSynchronize(ev_early));
    } else {
      CUADMM_HIP_TRY(hipStreamSynchronize(st));
    }
    prof_collect();
    return CUADMM_OK;
  }

  int launch_aty(bool write_xb) {
    prof_begin(K_ATY);
    int rc = launch_aty_xb(write_xb, L, At_rp.p, At_ci.p, At_v.p, y_d.p, C.p, X.p, sig, Rd1.p, Xb.p, st, &At_long);
    prof_end(K_ATY, (write_xb ? 32.0 : 16.0) * (double)L + 4.0 * (double)L);
    return rc;
  }
  // after_fused: the local rows were written by the fused projection kernels of this step -- only the other rows are left
  int launch_spmv(bool doX, bool doS, bool after_fused = false) {
    if (!(after_fused && lrows.active && lrows.nrest == 0)) closed.out_dirty = true;
    if (after_fused && lrows.active) {
      if (lrows.nrest == 0) return CUADMM_OK;
      prof_begin(K_SPMV);
      int rc = launch_spmv_rows(lrows.nrest, lrows.rest_avg, lrows.rest_rp.p, lrows.rest_ci.p, lrows.rest_v.p, X.p, S.p, C.p, doX ? out_w : nullptr,
                                doS ? out_w + m + 2 : nullptr, st, nullptr, lrows.rest_map.p);
      prof_end(K_SPMV, 12.0 * (double)lrows.rest_v.n + 8.0 * lrows.nrest * ((doX ? 1 : 0) + (doS ? 1 : 0)));
      return rc;
    }
    prof_begin(K_SPMV);
    int rc = launch_spmv_rows(m, A_avg_nnz, A_rp.p, A_ci.p, A_v.p, X.p, S.p, C.p, doX ? out_w : nullptr,
                              doS ? out_w + m + 2 : nullptr, st, &A_long);
    prof_end(K_SPMV, 12.0 * (double)A_v.n + 8.0 * m * ((doX ? 1 : 0) + (doS ? 1 : 0)));
    return rc;
  }
  int launch_project() {
    prof_begin(K_PSD);
    int rc = plan.project(Xb.p, Xproj.p, st);
    prof_end(K_PSD, 16.0 * (double)L);
    return rc;
  }
  // Step 2 of a fused iteration: Rd1 / Xb on the rest of the svec, then the projection whose fused blocks also do the
  // post step `mode` (0: S, X, sums; 1: S only) on their own ranges, then the post step on the rest (+ the sums).
  int launch_fused_step(int mode, double tau, int iters = 1) {
    int rc;
    prof_begin(K_ATY);
    rc = launch_aty_xb_idx(plan.n_rest, plan.d_rest, At_rp.p, At_ci.p, At_v.p, y_d.p, C.p, X.p, sig, Rd1.p, Xb.p, st);
    prof_end(K_ATY, 36.0 * (double)plan.n_rest);
    if (rc) return rc;
    SignFuse fz{};                                     // every optional part (local rows, closed blocks) off
    fz.rp = At_rp.p; fz.ci = At_ci.p; fz.av = At_v.p; fz.y = y_d.p; fz.C = C.p;
    fz.X = X.p; fz.Rd1 = Rd1.p; fz.S = S.p; fz.partials = partials.p;
    fz.sig = sig; fz.inv_sig = 1 / sig; fz.tau_sig = tau * sig; fz.mode = mode;
    if (lrows.active) {
      fz.lc = lrows.desc.p; fz.lc_row = lrows.row.p; fz.lc_nzptr = lrows.nzptr.p; fz.lc_e = lrows.e.p; fz.lc_v = lrows.v.p;
      fz.outX = mode == 0 ? out_w : nullptr;
      fz.outS = out_w + m + 2;
    }
    if (closed.active) {
      fz.rec = closed.rec.p; fz.cl_out = closed.cl_out.p; fz.y_out = y_d.p;
      fz.iter0 = (int)(closed.iters_done & 0x3fffffff);
      closed.iters_done += iters > 1 ? iters : 1;
      fz.partials2 = closed.partials2.p;
      fz.isig = 1 / sig; fz.bscale = bscale;
      if (closed.out_dirty) {
        if ((rc = launch_closed_gather_out(closed.rec.p, plan.fused_blocks(), out_d.p, out_d.p + (size_t)m + 2, closed.cl_out.p, st))) return rc;
        closed.out_dirty = false;
      }
    }
    if (iters > 1) {   // batch: every block is closed and fused (can_batch), nothing runs beside the projection launches
      fz.iters = iters; fz.pstride = bt.pstride; fz.partials = bt.p1.p; fz.partials2 = bt.p2.p;
      prof_begin(K_PSD);
      rc = plan.project(Xb.p, Xproj.p, st, &fz);
      prof_end(K_PSD, 68.0 * (double)L * iters);
      if (rc) return rc;
      prof_begin(K_POST);
      double* dst = (!dev_scalars && bt.h_dev) ? bt.h_dev : bt.scal_d.p;
      rc = launch_reduce_quads_batch(bt.p1.p, bt.p2.p, plan.fused_blocks(), bt.pstride, iters, dst, st);
      prof_end(K_POST, 0.0);
      if (rc) return rc;
      if (dev_scalars && (rc = comm_allreduce(bt.scal_d.p, 4 * (size_t)iters))) return rc;
      if (dst == bt.scal_d.p) CUADMM_HIP_TRY(hipMemcpyAsync(bt.h.p, bt.scal_d.p, sizeof(double) * 4 * (size_t)iters, hipMemcpyDeviceToHost, st));
      bt.launches++; bt.iters += iters;
      return CUADMM_OK;
    }
    prof_begin(K_PSD);
    rc = plan.project(Xb.p, Xproj.p, st, &fz);
    prof_end(K_PSD, 68.0 * (double)(L - plan.n_rest) + 16.0 * (double)plan.n_rest);
    if (rc) return rc;
    prof_begin(K_POST);
    stats_fused = closed.active && mode == 0;
    int nparts = 0;
    rc = launch_post_rest(mode, plan.n_rest, plan.d_rest, plan.fused_blocks(), Xproj.p, Rd1.p, C.p, X.p, S.p, 1 / sig, tau * sig, partials.p,
                          out_w + (size_t)m, st, stats_fused ? &nparts : nullptr);
    if (!rc && stats_fused) {   // all four scalars of the stopping test in one launch (rp_stats is not needed this iteration)
      double* dst = (!dev_scalars && h_scal_dev) ? h_scal_dev : scal_d.p;
      if (!quad_seg.p && reduce_quads_segments(nparts, plan.fused_blocks()) > 1 && (rc = quad_seg.alloc(4 * (size_t)reduce_quads_segments(nparts, plan.fused_blocks()) + 4))) return rc;
      rc = launch_reduce_quads(partials.p, nparts, closed.partials2.p, plan.fused_blocks(), dst, out_w + (size_t)m, quad_seg.p, st);
    }
    prof_end(K_POST, (mode == 0 ? 48.0 : 32.0) * (double)plan.n_rest);
    return rc;
  }
  // --- several iterations per launch ---------------------------------------------------------------------------------
  bool can_batch() const {
    return can_batch_local() && bt.peers_agree && aa.mem == 0 && inf.period == 0 && lb.period == 0;
  }
  bool can_batch_local() const {
    return bt.max_iters >= 2 && fuse && closed.active && dev_solve && !lead.ready && plan.n_rest == 0 && eig_rank == 0 && !out_mapped &&
           plan.fused_blocks() > 0 && (bt.allow_mixed || plan.one_dominant_geometry());
  }
  // Ranks must take the batching decision TOGETHER: it decides which collective a rank issues (shards of a heterogeneous problem
  // can differ: no dominant geometry on one, a block with more than 8 rows on another, no blocks at all on a third).  One small
  // all-reduce at the start of every solve (options may have changed since the last one).
  int batch_agree() {
    bt.peers_agree = true;
    const int cw = local_mode ? comm_world : world;
    if (cw <= 1 && !force_comm) return CUADMM_OK;
    if (!allreduce && !rccl_comm) return CUADMM_OK;      // no transport yet: the first collective of the solve reports it
    h_scal.p[0] = can_batch_local() ? 1.0 : 0.0;
    h_scal.p[1] = 1.0;
    CUADMM_HIP_TRY(hipMemcpyAsync(scal_d.p, h_scal.p, sizeof(double) * 2, hipMemcpyHostToDevice, st));
    int rc = comm_allreduce(scal_d.p, 2);
    if (rc) return rc;
    CUADMM_HIP_TRY(hipMemcpyAsync(h_scal.p, scal_d.p, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
    CUADMM_HIP_TRY(hipStreamSynchronize(st));
    bt.peers_agree = h_scal.p[0] >= h_scal.p[1] - 0.5;    // every rank said yes
    return CUADMM_OK;
  }
  int batch_alloc() {
    // sized for the CURRENT option value: "batch" may be raised between solves, and a launch of K iterations writes K partial
    // arrays and 4 K scalars
    if (bt.p1.p && bt.cap >= bt.max_iters) return CUADMM_OK;
    bt.pstride = 2 * (long long)plan.fused_blocks() + 2;
    bt.cap = 0; bt.h_dev = nullptr;
    int rc;
    if ((rc = bt.p1.alloc((size_t)bt.pstride * bt.max_iters)) || (rc = bt.p2.alloc((size_t)bt.pstride * bt.max_iters)) ||
        (rc = bt.scal_d.alloc(4 * (size_t)bt.max_iters)) || (rc = bt.h.alloc(4 * (size_t)bt.max_iters)))
      return rc;
    if (!bt.ck_X.p && ((rc = bt.ck_X.alloc(L)) || (rc = bt.ck_S.alloc(L)) || (rc = bt.ck_y.alloc(std::max(m, 1))) || (rc = bt.ck_out.alloc(2 * (size_t)m + 2))))
      return rc;
    bt.cap = bt.max_iters;
    void* dp = nullptr;
    if (sw.mapped_out && hipHostGetDevicePointer(&dp, bt.h.p, 0) == hipSuccess && dp) bt.h_dev = static_cast<double*>(dp);
    else { hipError_t e = hipGetLastError(); (void)e; }
    return CUADMM_OK;
  }
  int batch_copy(bool save) {   // checkpoint of everything an iteration reads and writes: X, S, y, [A X | sums | A (S - C)]
    prof_begin(K_COPY);
    struct { double* live; double* ck; size_t n; } v[4] = {{X.p, bt.ck_X.p, (size_t)L}, {S.p, bt.ck_S.p, (size_t)L}, {y_d.p, bt.ck_y.p, (size_t)m},
                                                           {out_d.p, bt.ck_out.p, 2 * (size_t)m + 2}};
    CopyJobs jobs{};                       // ONE launch for the whole checkpoint (five copies of ~0.03 ms each were 1.3 % of a batch of 44)
    for (auto& q : v) {
      jobs.dst[jobs.count] = save ? q.ck : q.live; jobs.src[jobs.count] = save ? q.live : q.ck; jobs.nbytes[jobs.count] = (long long)(q.n * sizeof(double));
      ++jobs.count;
    }
    if (hint_d.p) {   // the schedule hints are part of the state an iteration reads and writes
      if (!bt.ck_hint.p) { int rc = bt.ck_hint.alloc(hint_d.n); if (rc) return rc; }
      jobs.dst[jobs.count] = save ? bt.ck_hint.p : hint_d.p; jobs.src[jobs.count] = save ? hint_d.p : bt.ck_hint.p; jobs.nbytes[jobs.count] = (long long)(sizeof(int) * hint_d.n);
      ++jobs.count;
    }
    { int rc = launch_copy_multi(jobs, st); if (rc) return rc; }
    if (save) bt.ck_iters_done = closed.iters_done; else closed.iters_done = bt.ck_iters_done;
    prof_end(K_COPY, 16.0 * (2.0 * (double)L + 3.0 * m + 2));
    return CUADMM_OK;
  }
  // the device ran bt.len iterations, the host schedule accepts only the first `keep` of them: back to the checkpoint and
  // forward again by `keep` iterations (bit-identical: same kernels, same inputs)
  int batch_rollback(int keep) {
    if (!bt.have_ck) { set_error("internal: batch invalidated without a checkpoint"); return CUADMM_ERR_INVALID; }
    int rc = batch_copy(false);
    if (rc) return rc;
    closed.out_dirty = true;
    const double sig_now = sig;
    sig = bt.sig;
    if (keep == 1) rc = launch_fused_step(0, bt.tau);
    else if (keep > 1) rc = launch_fused_step(0, bt.tau, keep);
    sig = sig_now;
    if (rc) return rc;
    CUADMM_HIP_TRY(hipStreamSynchronize(st));
    prof_collect();
    stats_fused = false;
    bt.len = bt.pos = 0;
    bt.rollbacks++;
    return CUADMM_OK;
  }
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

  int launch_post_mode(int mode, double tau) {
    prof_begin(K_POST);
    int rc = launch_post(mode, L, Xproj.p, Rd1.p, C.p, X.p, S.p, 1 / sig, tau * sig, partials.p, out_w + (size_t)m, st);
    prof_end(K_POST, (mode == 0 ? 48.0 : (mode == 1 ? 32.0 : 40.0)) * (double)L);
    return rc;
  }
};

using Solver = cuadmm_solver;

// keeps the calling thread's current device across an entry point that visits several devices (the in-process group's leader):
// a caller that shares the thread with another HIP user (torch) finds its device as it left it
struct DeviceGuard {
  int dev = -1;
  DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) { dev = -1; (void)hipGetLastError(); } }
  ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// `in_group_call` marks the calls an in-process group (duo_group.hip) makes on its own ranks, rank 0 -- the leader itself -- included
template <class F>
static int as_group_rank(cuadmm_solver* q, F&& call) {
  q->in_group_call = true;
  const int rc = call(q);
  q->in_group_call = false;
  return rc;
}
// the leader forwards an entry point: every rank runs `call`, ranks >= 1 on their own host threads
template <class F>
static int group_forward(cuadmm_solver* s, F&& call) {
  DeviceGuard keep_device;                  // the ranks' devices are made current on this thread: leave the caller's as it was
  return duo_group_run(s->group, [&](cuadmm_solver* q, int) { return as_group_rank(q, call); });
}

static int check_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    set_error("no HIP device available (hipGetDeviceCount: %s); this engine has no CPU fallback", hipGetErrorString(e));
    return CUADMM_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= n) { set_error("device %d out of range (0..%d)", device, n - 1); return CUADMM_ERR_NO_DEVICE; }
  CUADMM_HIP_TRY(hipSetDevice(device));
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// SDPSolver::init, in stages.  InitIn: the caller's arrays (solver.h:208-223); InitCtx: what one stage leaves for the next.
// ------------------------------------------------------------------------------------------
namespace {
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

// max(1, ||v[lo, hi)||): what a constraint's column is divided by (get_normA, sparse_matrix_norm.cu:11-31)
static double cons_norm(const double* v, int lo, int hi) {
  double nrm = 0.0;
  for (int p = lo; p < hi; ++p) nrm += v[p] * v[p];
  return std::max(1.0, std::sqrt(nrm));
}

static double sum_sq(const double* v, int n) {
  double t = 0;
  for (int i = 0; i < n; ++i) t += v[i] * v[i];
  return t;
}
// the indices of a sparse vector (`what` of entry point `who`): inside [0, n), none twice (the norms would count both entries, the vector one)
static int check_sparse_idx(const char* who, const char* what, const int* idx, int nnz, long long n) {
  std::vector<char> seen((size_t)n, 0);
  for (int i = 0; i < nnz; ++i) {
    if (idx[i] < 0 || idx[i] >= n) { set_error("%s: %s index %d out of range", who, what, idx[i]); return CUADMM_ERR_INVALID; }
    if (seen[idx[i]]) { set_error("%s: %s index %d appears twice", who, what, idx[i]); return CUADMM_ERR_INVALID; }
    seen[idx[i]] = 1;
  }
  return CUADMM_OK;
}
// sum (val_i / norm[idx_i])^2 over the entries, in their order (sparse_dense.cu:11-20)
static double sum_scaled_sq(const int* idx, const double* val, int nnz, const double* norm) {
  double t = 0;
  for (int i = 0; i < nnz; ++i) { const double v = val[i] / norm[idx[i]]; t += v * v; }
  return t;
}
// full[j] = val_i / normA[j] for the entries of this rank (j = g2l[idx_i], -1: another rank's; g2l null: j = idx_i); returns their sum of squares
static double scaled_b(const int* idx, const double* val, int nnz, const int* g2l, const std::vector<double>& normA, std::vector<double>& full) {
  double t = 0;
  full.assign(normA.size(), 0.0);
  for (int i = 0; i < nnz; ++i) {
    const int j = g2l ? g2l[idx[i]] : idx[i];
    if (j < 0) continue;
    const double v = val[i] / normA[j];
    full[j] = v;
    t += v * v;
  }
  return t;
}

#define CUADMM_INIT_STAGE_PROLOGUE \
  const int vec_len = in.vec_len, con_num = in.con_num, At_nnz = in.At_nnz, b_nnz = in.b_nnz, C_nnz = in.C_nnz, mat_num = in.mat_num; \
  const int *At_cp = in.At_cp, *At_ri = in.At_ri, *b_idx = in.b_idx, *C_idx = in.C_idx, *blk = in.blk; \
  const double *At_vx = in.At_vx, *b_vals = in.b_vals, *C_vals = in.C_vals, *X0 = in.X0, *y0 = in.y0, *S0 = in.S0; \
  const double sig = in.sig; \
  const int m = con_num; \
  const long long Lf = vec_len, L = s->L; \
  std::vector<double>&vals = c.vals, &rv = c.rv; \
  std::vector<int>&rp = c.rp, &rci = c.rci; \
  int rc = CUADMM_OK; \
  (void)vec_len; (void)At_nnz; (void)b_nnz; (void)C_nnz; (void)mat_num; (void)At_cp; (void)At_ri; (void)b_idx; (void)C_idx; (void)blk; (void)At_vx; \
  (void)b_vals; (void)C_vals; (void)X0; (void)y0; (void)S0; (void)sig; (void)m; (void)Lf; (void)L; (void)vals; (void)rv; (void)rp; (void)rci; \
  (void)0;

// stage: stream, events, global dimensions
static int init_device(Solver* s, const InitIn& in, InitCtx& c) {
  CUADMM_INIT_STAGE_PROLOGUE
  if ((rc = check_device(s->device))) return rc;
  s->t_init0 = wall_s();                                  // the reference's timer starts in init (solver.cu:41-44)
  CUADMM_HIP_TRY(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
  if (s->profile)
    for (int k = 0; k < K_NUM; ++k)
      for (int j = 0; j < 2; ++j) { CUADMM_HIP_TRY(hipEventCreate(&s->ev0[k][j])); CUADMM_HIP_TRY(hipEventCreate(&s->ev1[k][j])); }

  s->m = m; s->L_full = vec_len; s->nblk_full = mat_num; s->sig = sig;

  return rc;
}

// stage: get_normA and A^T in CSR over the svec rows (what the factor and the device matrices are built from)
static int init_normalise(Solver* s, const InitIn& in, InitCtx& c) {
  CUADMM_INIT_STAGE_PROLOGUE
  // --- get_normA (sparse_matrix_norm.cu:11-31): norm_j = max(1,||col j||), column scaled in place
  vals.assign(At_vx, At_vx + At_nnz);
  if (!s->upa.in_update) { s->upa.cp.assign(At_cp, At_cp + m + 1); s->upa.ri.assign(At_ri, At_ri + At_nnz); }
  s->normA.assign(m, 1.0);
  for (int j = 0; j < m; ++j) {
    const double nrm = cons_norm(vals.data(), At_cp[j], At_cp[j + 1]);
    s->normA[j] = nrm;
    for (int p = At_cp[j]; p < At_cp[j + 1]; ++p) vals[p] /= nrm;
  }

  // --- At in CSR over the svec rows (== CSC of A), solver.cu:83-88
  rp.assign((size_t)Lf + 1, 0); rci.assign((size_t)At_nnz, 0);
  rv.assign((size_t)At_nnz, 0.0);
  for (int p = 0; p < At_nnz; ++p) rp[(size_t)At_ri[p] + 1]++;
  for (long long i = 0; i < Lf; ++i) rp[i + 1] += rp[i];
  {
    std::vector<int> pos(rp.begin(), rp.end() - 1);
    for (int j = 0; j < m; ++j)
      for (int p = At_cp[j]; p < At_cp[j + 1]; ++p) {
        int q = pos[At_ri[p]]++;
        rci[q] = j; rv[q] = vals[p];
      }
  }

  return rc;
}

// The probe solve of a freshly built GPU tail (init, and cuadmm_update_A after it rebuilt the tail): see init_factor
static int tail_probe(Solver* s, const int64_t* srp, const int* sci, const double* sv, int tk, bool& tail_ok) {
  int rc = CUADMM_OK;
  std::vector<double> x((size_t)tk), z((size_t)tk, 0.0), r((size_t)tk, 0.0);
  unsigned long long seed = 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < tk; ++i) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; x[i] = 0.5 + (double)(seed >> 11) * (1.0 / 9007199254740992.0); }
  auto apply_S = [&](const std::vector<double>& in, std::vector<double>& out) {
    std::fill(out.begin(), out.end(), 0.0);
    for (int i = 0; i < tk; ++i)
      for (int64_t q = srp[i]; q < srp[i + 1]; ++q) {
        const int j = sci[q];
        out[i] += sv[q] * in[j];
        if (j != i) out[j] += sv[q] * in[i];
      }
  };
  apply_S(x, z);
  std::vector<double> xh = z;
  rc = s->tail.solve(xh.data(), s->st);
  apply_S(xh, r);
  double err = 0, zn = 0;
  for (int i = 0; i < tk; ++i) { err = std::max(err, std::fabs(r[i] - z[i])); zn = std::max(zn, std::fabs(z[i])); }
  tail_ok = rc == CUADMM_OK && err <= 1e-6 * zn;
  if (!tail_ok && rc == CUADMM_OK && s->verbose)
    printf("\n A*A^T factor: the GPU tail of size %d fails its probe solve (backward error %.1e): falling back to the host-only factor\n", tk, err / std::max(zn, 1e-300));
  return rc;
}

// stage: A A^T + eps I: ordering, host factor, GPU tail of the Schur complement with its probe solve, permutation
static int init_factor(Solver* s, const InitIn& in, InitCtx& c) {
  CUADMM_INIT_STAGE_PROLOGUE
  // --- factor of A A^T + 1e-15 I (solver.cu:91-96, cholesky_cpu.h:62-141): ordering, symbolic analysis and the sparse
  // leading columns on the host; when the cost model finds a dense tail, its Schur complement is factored (dense
  // LDL^T with diagonal pivoting) and inverted on the GPU, and x = W^T D^-1 W z is applied in ONE pass over W = inv(L22)
  // per solve (tail_solve.hip; the two triangular GEMVs remain as the fallback and behind option tail_one_pass = 0).
  // CUADMM_TAIL_K: 0 = everything on the host, k > 0 forces the tail size (A/B measurements).
  {
    int max_k = std::max(64, std::min(s->sw.tail_max_k, 65536));
    if (s->sw.tail_k >= 0) max_k = -std::min(std::min(s->sw.tail_k, m), 65536);
    double t0 = wall_s();
    s->upa.orderings++;
    if (max_k == 0) rc = cuadmm_aat_create(m, vec_len, rp.data(), rci.data(), rv.data(), 1e-15, &s->fac);
    else {
      // the planner may choose a (smaller) tail for the solve with dense tree tops unless the options rule that solve out
      cuadmm_aat_plan_allow_tops(s->sw.lead_tops != 0 && !s->sw.host_solve && s->sw.l21_device != 2);
      rc = cuadmm_aat_create_split(m, vec_len, rp.data(), rci.data(), rv.data(), 1e-15, max_k, &s->fac);
      cuadmm_aat_plan_allow_tops(1);
    }
    if (rc) return rc;
    double t1 = wall_s();
    int tk = cuadmm_aat_tail_k(s->fac);
    if (tk > 0) {
      const int64_t* srp; const int* sci; const double* sv;
      rc = cuadmm_aat_tail_schur(s->fac, &srp, &sci, &sv);
      s->tail.one_pass = s->sw.tail_one_pass != 0;
      s->tail.refine = s->sw.tail_refine != 0;
      s->tail.pivot = s->sw.tail_pivot != 0;
      if (!rc) rc = s->tail.build_from_schur(reinterpret_cast<const long long*>(srp), sci, sv, tk, s->st);
      // The tail is applied as an explicit inverse built without pivoting (tail_solve.hip); with (nearly) dependent
      // constraints the pivots approach the regularisation 1e-15 and inv(L22) could lose accuracy silently.  Probe it with
      // a consistent right-hand side z = S x (S = the Schur complement the tail factors, lower triangle with diagonal):
      // solve on the GPU and check the BACKWARD error ||S x^ - z|| / ||z|| -- the forward error is meaningless here (moment
      // relaxations have numerically singular S: no solver recovers x, and the ADMM iteration only needs a small residual).
      // On failure fall back to the host-only factor (CHOLMOD-style substitution, no explicit inverse).
      bool tail_ok = rc == CUADMM_OK;
      if (rc == CUADMM_OK) rc = tail_probe(s, srp, sci, sv, tk, tail_ok);
      cuadmm_aat_tail_schur_release(s->fac);
      if (rc && rc != CUADMM_ERR_FACTOR) return rc;
      if (!tail_ok) {
        s->tail.release();
        cuadmm_aat_free(s->fac);
        s->fac = nullptr;
        s->upa.orderings++; s->upa.tail_fellback = true;
        if ((rc = cuadmm_aat_create(m, vec_len, rp.data(), rci.data(), rv.data(), 1e-15, &s->fac))) return rc;
      }
    }
    tk = s->tail.k;
    // a rank of a sharded engine keeps only the rows of inv(L22) it applies (TailSolve::keep_shard; the reference splits its buffers over the
    // devices too, src/duo_solver.cu:269-295): 1 / world of the triangle per rank instead of W and W^T whole
    if (tk > 0 && s->world > 1 && !s->local_mode && s->sw.tail_shard != 0 && !s->sw.tail_refine && (rc = s->tail.keep_shard(s->rank, s->world, s->st))) return rc;
    if (s->verbose) {
      const long long lnz = (long long)cuadmm_aat_factor_nnz(s->fac);
      if (tk > 0)
        printf("\n A*A^T factor: nnz(L) = %lld; host part %.2fs; last %d of %d columns (%.1f%% of nnz(L)) factored and inverted on the GPU in %.2fs\n",
               lnz, t1 - t0, tk, m, 100.0 * (double)(lnz - cuadmm_aat_factor_colptr(s->fac)[m - tk]) / (double)std::max<long long>(1, lnz), s->tail.build_s);
      else
        printf("\n A*A^T factor: nnz(L) = %lld on the host in %.2fs\n", lnz, t1 - t0);
    }
  }
  s->perm.assign(cuadmm_aat_perm(s->fac), cuadmm_aat_perm(s->fac) + m);
  s->perm_inv.assign(m, 0);
  for (int i = 0; i < m; ++i) s->perm_inv[s->perm[i]] = i;

  return rc;
}

// stage: census, this rank's block range, the projection plan (closed-block candidate, schedule hints, step counts)
static int init_plan(Solver* s, const InitIn& in, InitCtx& c) {
  CUADMM_INIT_STAGE_PROLOGUE
  // --- census (analyze_blk.cu:63-99, matrix_sizes.cu:75-113)
  if (s->verbose) {
    std::vector<int> sizes, nums;
    std::vector<int> psd_blk;
    for (int k = 0; k < mat_num; ++k) if (blk[k] > 0) psd_blk.push_back(blk[k]);
    analyze_blk(psd_blk.data(), (int)psd_blk.size(), sizes, nums);
    print_blk_census(sizes, nums);
    MatrixSizes ms;
    ms.init(sizes, nums);
    ms.print();
  }

  // --- shard: contiguous block range of this rank
  std::vector<int> first;
  partition_blocks(blk, mat_num, s->world, first);
  s->blk_begin = first[s->rank]; s->blk_end = first[s->rank + 1];
  long long off = 0;
  s->sv_begin = 0;
  for (int k = 0; k < mat_num; ++k) {
    if (k == s->blk_begin) s->sv_begin = off;
    off += blk_svec_len(blk[k]);
    if (k + 1 == s->blk_end) s->sv_end = off;
  }
  if (s->blk_begin == s->blk_end) { s->sv_begin = s->sv_end = (s->blk_begin == mat_num ? off : s->sv_begin); }
  s->L = s->sv_end - s->sv_begin;
  s->blk_local.assign(blk + s->blk_begin, blk + s->blk_end);
  s->plan.eig_rank = s->eig_rank > 0 ? s->eig_rank : 0;
  {
    // Closed-block candidate: every constraint lives in ONE block of this rank, no block has more than kClosedMaxRows of them or
    // more than kFuseRowsMax nonzeros, every block fits a one-wavefront kernel (n <= 64).  Then the tiny blocks go through the sign
    // kernel too (PsdPlan::tiny_sign), so that the whole iteration of every block can run in psd_sign_closed.h.
    const auto& bl = s->blk_local;
    bool cand = s->opt_tiny_sign != 0 && s->eig_rank == 0 && !bl.empty() && m > 0 && s->world == 1;
    bool any_tiny = false;
    for (size_t k = 0; k < bl.size() && cand; ++k) { cand = bl[k] > 0 && bl[k] <= 64; any_tiny = any_tiny || bl[k] <= 8; }
    if (cand && any_tiny && s->opt_tiny_sign == 1) {
      std::vector<long long> boff(bl.size() + 1, 0);
      for (size_t k = 0; k < bl.size(); ++k) boff[k + 1] = boff[k] + blk_svec_len(bl[k]);
      std::vector<int> rows_of(bl.size(), 0), nz_of(bl.size(), 0);
      for (int j = 0; j < m && cand; ++j) {
        if (At_cp[j] == At_cp[j + 1]) continue;
        const long long r0 = At_ri[At_cp[j]];
        const size_t k = (size_t)(std::upper_bound(boff.begin(), boff.end(), r0) - boff.begin()) - 1;
        for (int p = At_cp[j]; p < At_cp[j + 1] && cand; ++p) cand = At_ri[p] >= boff[k] && At_ri[p] < boff[k + 1];
        cand = cand && ++rows_of[k] <= kClosedMaxRows && (nz_of[k] += At_cp[j + 1] - At_cp[j]) <= kFuseRowsMax;
      }
    }
    s->plan.tiny_sign = cand && any_tiny;
    s->closed_candidate = cand;
  }
  rc = s->plan.build(s->blk_local.data(), (int)s->blk_local.size());
  s->plan.overlap = true;
  if (!rc && !s->blk_local.empty() && s->opt_hint != 0) {
    // Schedule warm start of the ONE-WAVEFRONT sign kernels (lift steps each block needed in the previous projection): C2 12.0 ->
    // 11.4 steps (+3 % iterations / s), C4 11.0 -> 10.5.  On the batched-GEMM path for the mid-size blocks only (groups padded to <= 512,
    // psd_large.h; psd_hint = 2: every group): one n = 2 000 block loses a step (C3: 17 -> 18 -- the recorded count includes the overshoot
    // of the previous run's bursts, and a failed first probe costs 4 steps there).
    // The hint ages by one step every 16th projection (PsdPlan::project; inside the task loop of the batched launches).
    if ((rc = s->hint_d.alloc(s->blk_local.size()))) return rc;
    CUADMM_HIP_TRY(hipMemset(s->hint_d.p, 0, sizeof(int) * s->blk_local.size()));
    s->plan.d_hint = s->hint_d.p;
    s->plan.sign.d_hint = s->hint_d.p;
    s->plan.sign.hint_max_n = s->opt_hint == 2 ? (1 << 30) : (s->opt_hint == 3 ? 0 : 512);      // 3: the one-wavefront kernels only (rounds 2 - 4)
  }
  // step counts per block: for cuadmm_get_psd_steps and for the longest-block-first reordering of the fused launches
  if (!rc && (s->psd_steps || s->plan.fusable()) && !s->blk_local.empty()) {
    if ((rc = s->steps_d.alloc(s->blk_local.size()))) return rc;
    CUADMM_HIP_TRY(hipMemset(s->steps_d.p, 0, sizeof(int) * s->blk_local.size()));
    s->plan.d_steps = s->steps_d.p;
    s->plan.sign.d_steps = s->steps_d.p;
  }
  if (rc) return rc;

  return rc;
}

// stage: A^T and A on the device with the permutation folded in; which blocks fuse, which constraint rows are local to one
static int init_matrices(Solver* s, const InitIn& in, InitCtx& c) {
  CUADMM_INIT_STAGE_PROLOGUE
  // --- device matrices with the permutation folded in
  {
    std::vector<int> lrp((size_t)L + 1, 0), lci;
    std::vector<double> lv;
    const int base = rp[s->sv_begin];
    const int cnt = rp[s->sv_end] - base;
    lci.resize(cnt); lv.resize(cnt);
    for (long long i = 0; i <= L; ++i) lrp[i] = rp[s->sv_begin + i] - base;
    for (int q = 0; q < cnt; ++q) { lci[q] = s->perm_inv[rci[base + q]]; lv[q] = rv[base + q]; }
    if ((rc = s->At_long.build(L, lrp.data()))) return rc;
    if ((rc = s->At_rp.from(lrp)) || (rc = s->At_ci.from(lci)) || (rc = s->At_v.from(lv))) return rc;
    // A rows in permuted order, local columns
    std::vector<int> arp((size_t)m + 1, 0), aci;
    std::vector<double> av;
    aci.reserve(cnt); av.reserve(cnt);
    for (int pidx = 0; pidx < m; ++pidx) {
      const int j = s->perm[pidx];
      for (int p = At_cp[j]; p < At_cp[j + 1]; ++p) {
        const long long r = At_ri[p];
        if (r >= s->sv_begin && r < s->sv_end) { aci.push_back((int)(r - s->sv_begin)); av.push_back(vals[p]); }
      }
      arp[pidx + 1] = (int)aci.size();
    }
    if ((rc = s->A_long.build(m, arp.data()))) return rc;
    s->A_avg_nnz = spmv_avg_nnz(m, arp.data(), s->A_long);   // long rows count with their capped part only
    // fused iteration: needs the one-wavefront-per-block sign kernels and no long rows of A^T (they are summed by their own kernel)
    s->fuse = s->plan.fusable() && s->At_long.nlong == 0 && !s->sw.debug_eig && s->sw.fuse != 0;
    s->lrows.active = false; s->lrows.nlocal = s->lrows.nrest = 0;
    if (s->fuse && s->A_long.nlong == 0 && m > 0 && s->sw.fuse_rows != 0) {
      // constraint rows local to one fused block -> that block's kernel (psd_fuse.h)
      std::vector<int> slot_of;
      s->plan.fused_slots(slot_of);                                    // block -> partial-sum slot, -1: not fused
      const int nslots = s->plan.fused_blocks();
      std::vector<long long> boff((size_t)s->blk_local.size() + 1, 0);
      for (size_t k = 0; k < s->blk_local.size(); ++k) boff[k + 1] = boff[k] + blk_svec_len(s->blk_local[k]);
      std::vector<int> row_slot((size_t)m, -1);
      int nlocal = 0;
      for (int r = 0; r < m; ++r) {
        if (arp[r + 1] == arp[r]) continue;
        const long long c0 = aci[arp[r]];
        const int k = (int)(std::upper_bound(boff.begin(), boff.end(), c0) - boff.begin()) - 1;
        if (slot_of[k] < 0) continue;
        bool in = true;
        for (int p = arp[r]; p < arp[r + 1] && in; ++p) in = aci[p] >= boff[k] && aci[p] < boff[k + 1];
        if (!in) continue;
        row_slot[r] = slot_of[k];
      }
      {   // a block keeps its local rows only if one lane per row and one per nonzero suffice (psd_fuse.h)
        std::vector<long long> nz_of((size_t)nslots, 0), rows_of((size_t)nslots, 0);
        for (int r = 0; r < m; ++r) if (row_slot[r] >= 0) { nz_of[row_slot[r]] += arp[r + 1] - arp[r]; rows_of[row_slot[r]]++; }
        for (int r = 0; r < m; ++r) {
          if (row_slot[r] < 0) continue;
          if (nz_of[row_slot[r]] > kFuseRowsMax || rows_of[row_slot[r]] > kFuseRowsMax) { row_slot[r] = -1; continue; }
          ++nlocal;
        }
      }
      if (nlocal > 0) {
        // rows grouped by BLOCK (plan order of the blocks, rows ascending inside a block); lc[block] = {first row, rows |
        // longest row << 16, first nonzero, nonzeros}
        const size_t nb = s->blk_local.size();
        std::vector<int> blk_of_slot((size_t)nslots, -1);
        for (size_t k = 0; k < nb; ++k) if (slot_of[k] >= 0) blk_of_slot[slot_of[k]] = (int)k;
        std::vector<int> bcnt(nb + 1, 0);
        for (int r = 0; r < m; ++r) if (row_slot[r] >= 0) bcnt[(size_t)blk_of_slot[row_slot[r]] + 1]++;
        for (size_t k = 0; k < nb; ++k) bcnt[k + 1] += bcnt[k];
        std::vector<int> lrow((size_t)nlocal), lnz((size_t)nlocal + 1, 0), le, fill(bcnt.begin(), bcnt.end() - 1);
        std::vector<double> lval;
        for (int r = 0; r < m; ++r) if (row_slot[r] >= 0) lrow[fill[blk_of_slot[row_slot[r]]]++] = r;
        for (int q = 0; q < nlocal; ++q) {
          const int r = lrow[q];
          const long long base = boff[blk_of_slot[row_slot[r]]];
          for (int p = arp[r]; p < arp[r + 1]; ++p) { le.push_back((int)(aci[p] - base)); lval.push_back(av[p]); }
          lnz[q + 1] = (int)le.size();
        }
        std::vector<LcDesc> lcd(nb, LcDesc{0, 0, 0, 0});
        for (size_t k = 0; k < nb; ++k) {
          const int k0 = bcnt[k], k1 = bcnt[k + 1];
          int longest = 0;
          for (int q = k0; q < k1; ++q) longest = std::max(longest, lnz[q + 1] - lnz[q]);
          lcd[k] = LcDesc{k0, (k1 - k0) | (longest << 16), lnz[k0], lnz[k1] - lnz[k0]};
        }
        std::vector<int> rrp{0}, rci, rmap;
        std::vector<double> rv2;
        for (int r = 0; r < m; ++r) {
          if (row_slot[r] >= 0) continue;
          for (int p = arp[r]; p < arp[r + 1]; ++p) { rci.push_back(aci[p]); rv2.push_back(av[p]); }
          rrp.push_back((int)rci.size());
          rmap.push_back(r);
        }
        auto& lr = s->lrows;
        lr.nlocal = nlocal; lr.nrest = (int)rmap.size();
        lr.rest_avg = rmap.empty() ? 1.0 : (double)rci.size() / (double)rmap.size();
        lr.h_desc = lcd; lr.h_row = lrow; lr.h_nzptr = lnz; lr.h_e = le; lr.h_v = lval;
        if ((rc = lr.desc.from(lcd)) || (rc = lr.row.from(lrow)) || (rc = lr.nzptr.from(lnz)) || (rc = lr.e.from(le)) || (rc = lr.v.from(lval))) return rc;
        if (lr.nrest > 0) {
          if ((rc = lr.rest_rp.from(rrp)) || (rc = lr.rest_map.from(rmap)) || (rc = lr.rest_ci.alloc(std::max<size_t>(rci.size(), 1))) ||
              (rc = lr.rest_v.alloc(std::max<size_t>(rv2.size(), 1))) || (rc = lr.rest_ci.upload(rci.data(), rci.size())) ||
              (rc = lr.rest_v.upload(rv2.data(), rv2.size())))
            return rc;
        }
        lr.active = true;
      }
    }
    if ((rc = s->A_rp.from(arp)) || (rc = s->A_ci.alloc(std::max<size_t>(aci.size(), 1))) || (rc = s->A_v.alloc(std::max<size_t>(av.size(), 1)))) return rc;
    if ((rc = s->A_ci.upload(aci.data(), aci.size())) || (rc = s->A_v.upload(av.data(), av.size()))) return rc;
    s->A_v.n = av.size();
  }

  return rc;
}

// stage: scaling (solver.cu:169-191), b / C / X / S / y in the solver's units, work vectors
static int init_vectors(Solver* s, const InitIn& in, InitCtx& c) {
  CUADMM_INIT_STAGE_PROLOGUE
  // --- scaling (solver.cu:169-191)
  if ((rc = check_sparse_idx("init", "b", b_idx, b_nnz, m))) return rc;
  std::vector<double> bfull;
  double nb = sum_sq(b_vals, b_nnz), nc = sum_sq(C_vals, C_nnz), nb2 = scaled_b(b_idx, b_vals, b_nnz, nullptr, s->normA, bfull);
  if (s->local_mode) { nb = s->ov_nb; nb2 = s->ov_nb2; nc = s->ov_nc; }      // norms over ALL constraints / the whole C
  s->norm_borg = 1 + std::sqrt(nb);
  s->norm_Corg = 1 + std::sqrt(nc);
  s->upa.b_idx.assign(b_idx, b_idx + b_nnz); s->upa.b_val.assign(b_vals, b_vals + b_nnz);
  if (s->y_registered) {   // a second init on the same handle: the registration must not outlive the storage it names
    hipError_t e = hipHostUnregister(s->y_p.data()); (void)e;
    s->y_registered = false;
  }
  s->normA_p.resize(m); s->b_p.resize(m); s->y_p.assign(m, 0.0); s->Rp_p.assign(m, 0.0);
  s->y_best_p.assign(m, 0.0);
  if (m > 0 && hipHostRegister(s->y_p.data(), sizeof(double) * (size_t)m, hipHostRegisterDefault) == hipSuccess) s->y_registered = true;
  else { hipError_t e = hipGetLastError(); (void)e; }   // not fatal: upload_y then stages through the pinned buffer
  s->set_scaled_b(bfull, nb2);
  s->Cscale = 1 + std::sqrt(nc);
  s->objscale = s->bscale * s->Cscale;
  const double ibs = 1 / s->bscale, ics = 1 / s->Cscale;   // *_div_scalar multiply by 1/s (dense_scalar.cu:77-81)
  for (int pidx = 0; pidx < m; ++pidx) {
    const int j = s->perm[pidx];
    s->normA_p[pidx] = s->normA[j];
    if (y0) s->y_p[pidx] = (y0[j] * s->normA[j]) * ics;     // solver.cu:182,191
  }
  {
    std::vector<double> Cl((size_t)L, 0.0);
    std::vector<char> seen_C((size_t)L, 0);
    for (int i = 0; i < C_nnz; ++i) {
      if (C_idx[i] < 0 || C_idx[i] >= vec_len) { set_error("init: C index %d out of range", C_idx[i]); return CUADMM_ERR_INVALID; }
      if (C_idx[i] >= s->sv_begin && C_idx[i] < s->sv_end) {
        if (seen_C[C_idx[i] - s->sv_begin]) { set_error("init: C index %d appears twice", C_idx[i]); return CUADMM_ERR_INVALID; }
        seen_C[C_idx[i] - s->sv_begin] = 1;
        Cl[C_idx[i] - s->sv_begin] = C_vals[i] * ics;
      }
    }
    // kSvecPad: the closed-block kernels read whole batches of the flat svec walk past a block's last element without a
    // bounds clamp (psd_sign_closed.h); the values are never used
    if ((rc = s->C.from(Cl, kSvecPad))) return rc;
    std::vector<double> tmp((size_t)L, 0.0);
    if (X0) for (long long i = 0; i < L; ++i) tmp[i] = X0[s->sv_begin + i] * ibs;
    if ((rc = s->X.from(tmp, kSvecPad))) return rc;
    if (S0) for (long long i = 0; i < L; ++i) tmp[i] = S0[s->sv_begin + i] * ics;
    else std::fill(tmp.begin(), tmp.end(), 0.0);
    if ((rc = s->S.from(tmp, kSvecPad))) return rc;
  }
  if ((rc = s->Rd1.alloc(L)) || (rc = s->Xb.alloc(L)) || (rc = s->Xproj.alloc(L)) || (rc = s->y_d.alloc(std::max(m, 1))) ||
      (rc = s->out_d.alloc(2 * (size_t)m + 2)) || (rc = s->partials.alloc(2 * (size_t)post_grid(L) + 2 + 2 * (size_t)s->plan.fused_blocks())) ||
      (rc = s->h_out.alloc(2 * (size_t)m + 2)) || (rc = s->h_y.alloc(std::max(m, 1))) || (rc = s->scal_d.alloc(8 + 128)) ||
      (rc = s->h_scal.alloc(8)))
    return rc;
  CUADMM_HIP_TRY(hipMemset(s->out_d.p, 0, sizeof(double) * (2 * (size_t)m + 2)));
  std::memset(s->h_out.p, 0, sizeof(double) * (2 * (size_t)m + 2));
  s->out_w = s->out_d.p;
  if (s->fuse && (rc = s->plan.build_rest_index())) return rc;
  if (s->fuse && s->verbose)
    printf(" fused iteration: %d blocks form Xb and apply the S / X updates inside their projection kernel (%lld of %lld svec entries outside); "
           "%d of %d constraint rows are local to one of them\n", s->plan.fused_blocks(), s->plan.n_rest, L, s->lrows.nlocal, m);
  return rc;
}

// stage: where the y-solve runs: device-side sweeps around the GPU tail, one thread per tree of a block-diagonal factor, or the host
static int init_solve_plan(Solver* s, const InitIn& in, InitCtx& c) {
  CUADMM_INIT_STAGE_PROLOGUE
  s->dev_scalars = s->local_mode && s->comm_world > 1 && !s->sw.host_scalars;
  // device-side y-solve: whole factor on the host side of the split (no GPU tail) and a forest of many small trees
  s->dev_solve = false;
  if (s->tail.k > 0 && !s->sw.host_solve) {
    // split factor: leading sweeps on the device too when the leading elimination forest is shallow enough (cost model:
    // the deepest tree decides the kernel; host: 1.2 ns per leading nonzero for both sweeps + the PCIe hops of the tail)
    const int64_t* Lp; const int* Li; const double* Lx; const double* D;
    if ((rc = cuadmm_aat_factor_arrays(s->fac, &Lp, &Li, &Lx, &D))) return rc;
    s->lead.stream_only = s->sw.lead_stream != 0;
    s->lead.debug = s->sw.lead_debug != 0;
    s->lead.force_hybrid = s->sw.l21_device == 2;
    s->lead.small_kb = std::max(0, std::min(s->sw.lead_small_kb, 36));
    s->lead.tops_level = s->sw.l21_device == 2 ? 0 : (s->sw.lead_tops >= 0 ? s->sw.lead_tops : (cuadmm_aat_tail_tops(s->fac) > 0 ? cuadmm_aat_tail_tops(s->fac) : -1));
    if ((rc = s->lead.build(m, s->tail.k, Lp, Li, Lx, D, s->sw.l21_device != 0))) return rc;
    const double host_us = 1.2e-3 * (double)Lp[m - s->tail.k] + 150.0;
    if (s->lead.ready && s->lead.tops && !(s->lead.est_us < 0.7 * host_us)) {      // the cut forest loses to the host: the plain paths decide
      s->lead.tops_level = 0;
      if ((rc = s->lead.build(m, s->tail.k, Lp, Li, Lx, D, s->sw.l21_device != 0))) return rc;
    }
    if (s->lead.ready && s->lead.est_us < 0.7 * host_us) {
      s->dev_solve = true;
      if (s->local_mode && s->comm_world > 1) s->dev_scalars = true;
      if (s->verbose && s->lead.tops)
        printf(" y-solve on the device: sweeps over %d trees (depth <= %d), %d dense tree tops (%d columns, %.0f MB of inverses), the GPU tail\n", s->lead.ntrees,
               s->lead.max_levels, s->lead.tops_blocks, s->lead.nT, (double)s->lead.tops_bytes / 1e6);
      else if (s->verbose) printf(" y-solve on the device: leading sweeps over %d trees (depth <= %d) around the GPU tail\n", s->lead.ntrees, s->lead.max_levels);
    } else if (s->lead.hybrid || (s->lead.ready && s->sw.l21_device && s->lead.demote_to_hybrid())) {
      if (s->verbose) printf(" y-solve: L11 sweeps on the host (forest depth %d); L21 (%lld nonzeros) and the tail on the device\n", s->lead.max_levels, s->lead.nnz21);
    } else {
      s->lead.release();
    }
    // the planner sized the tail for the solve with dense tree tops; if that solve could not be built (an inverse failed its check, the
    // rest of the forest is still too deep) what runs instead is correct but slower than round 4's plan -- option lead_tops = 0 restores it
    if (cuadmm_aat_tail_tops(s->fac) > 0 && s->sw.lead_tops < 0 && !(s->dev_solve && s->lead.tops) && s->verbose)
      printf(" y-solve: the tail of %d columns was planned for dense tree tops, which could not be built (%s); option lead_tops = 0 plans without them\n",
             s->tail.k, cuadmm_last_error());
  }
  if (s->tail.k == 0 && m > 0 && !s->sw.host_solve) {
    int ntrees = 0, maxc = 0;
    const int *tp = nullptr, *tc = nullptr;
    if (cuadmm_aat_forest(s->fac, &ntrees, &maxc, &tp, &tc) == CUADMM_OK && ntrees >= 256 && maxc <= 64) {
      const int64_t* Lp; const int* Li; const double* Lx; const double* D;
      if ((rc = cuadmm_aat_factor_arrays(s->fac, &Lp, &Li, &Lx, &D))) return rc;
      const size_t lnz = (size_t)Lp[m];
      std::vector<long long> lp64(Lp, Lp + m + 1);
      if ((rc = s->f_tree_ptr.from(std::vector<int>(tp, tp + ntrees + 1))) || (rc = s->f_tree_cols.from(std::vector<int>(tc, tc + m))) ||
          (rc = s->f_Lp.from(lp64)) || (rc = s->f_Li.from(std::vector<int>(Li, Li + lnz))) || (rc = s->f_Lx.from(std::vector<double>(Lx, Lx + lnz))) ||
          (rc = s->f_D.from(std::vector<double>(D, D + m))))
        return rc;
      s->forest_trees = ntrees;
      s->dev_solve = true;
      if (s->local_mode && s->comm_world > 1) s->dev_scalars = true;
      if (s->verbose) printf(" y-solve on the device: %d independent trees of the elimination forest (<= %d columns each)\n", ntrees, maxc);
    }
  }
  return rc;
}

// stage: closed blocks: per-block records for psd_sign_closed.h
static int init_closed(Solver* s, const InitIn& in, InitCtx& c) {
  CUADMM_INIT_STAGE_PROLOGUE
  s->closed.active = false;
  // Default: only when no block with rows is smaller than 17 -- the solve adds two dependent memory round trips to a block's
  // prologue: < 4 % of the lifetime of an n >= 17 block (C2: 0.307 -> 0.300 ms per iteration, the solve and statistics kernels
  // gone), but 15 % of an n <= 16 block's (C4 with its 67 000 tiny blocks: 1.89 -> 1.91).  CUADMM_FUSE_SOLVE=1 / 0 forces it.
  // (round 2 kept blocks with rows and n < 17 out: the solve added two dependent round trips to their prologue; with the block
  // records of psd_sign_closed.h it rides in the one trip the prologue makes anyway)
  const bool want_closed = s->sw.fuse_solve != 0;
  if (want_closed && s->fuse && s->lrows.active && s->lrows.nrest == 0 && s->dev_solve && !s->lead.ready && s->forest_trees > 0 && s->lrows.nlocal == m) {
    const auto& hd = s->lrows.h_desc;
    const auto& hrow = s->lrows.h_row;
    const size_t nb = hd.size();
    bool ok = true;
    for (const auto& d : hd) ok = ok && (d.y & 0xffff) <= kClosedMaxRows;
    if (ok) {
      const int64_t* Lp; const int* Li; const double* Lx; const double* D;
      if ((rc = cuadmm_aat_factor_arrays(s->fac, &Lp, &Li, &Lx, &D))) return rc;
      std::vector<int> pos((size_t)m, -1), blk_of_row((size_t)m, -1);
      for (size_t k = 0; k < nb; ++k) {
        const int nk = hd[k].y & 0xffff;
        for (int q = 0; q < nk; ++q) { pos[hrow[hd[k].x + q]] = q; blk_of_row[hrow[hd[k].x + q]] = (int)k; }
      }
      // one ClosedRec per fused slot (psd_fuse.h): rows, their b / normA / D, the dense factor, the block's nonzeros of A in
      // local-row order with the round in which each is applied to its svec slot
      std::vector<int> slot_of;
      s->plan.fused_slots(slot_of);
      std::vector<ClosedRec> recs((size_t)std::max(s->plan.fused_blocks(), 1));
      std::memset(recs.data(), 0, sizeof(ClosedRec) * recs.size());
      for (auto& R : recs) for (int a = 0; a < kClosedMaxRows; ++a) R.D[a] = 1.0;     // rows >= nk: the kernel's sweeps run unmasked
      for (size_t k = 0; k < nb && ok; ++k) {
        if (slot_of[k] < 0) continue;
        ClosedRec& R = recs[(size_t)slot_of[k]];
        const int nk = hd[k].y & 0xffff;
        R.nk = nk; R.nnz = hd[k].w;
        if (R.nnz > kFuseRowsMax || nk > kClosedMaxRows) { ok = false; break; }
        for (int a = 0; a < nk && ok; ++a) {
          const int j = hrow[hd[k].x + a];
          R.rows[a] = j;
          R.D[a] = D[j]; R.b[a] = s->b_p[j]; R.normA[a] = s->normA_p[j];
          for (int64_t p = Lp[j]; p < Lp[j + 1]; ++p) {
            const int i = Li[p];
            if (blk_of_row[i] != (int)k || pos[i] <= a) { ok = false; break; }     // fill outside the block: not closed after all
            R.L[pos[i] * kClosedMaxRows + a] = Lx[p];
          }
        }
      }
      if (ok) {
        // nonzeros: s->lrows kept e / v / nzptr on the device only; rebuild them here from the host copies made above
        const auto& le = s->lrows.h_e; const auto& lval = s->lrows.h_v; const auto& lnz = s->lrows.h_nzptr;
        for (size_t k = 0; k < nb; ++k) {
          if (slot_of[k] < 0) continue;
          ClosedRec& R = recs[(size_t)slot_of[k]];
          const int k0 = hd[k].x, nk = R.nk, z0 = hd[k].z;
          int maxmult = 0;
          for (int a = 0; a <= nk; ++a) R.nzp[a] = (unsigned char)(lnz[k0 + a] - z0);
          for (int a = 0; a < nk; ++a) R.maxlen = std::max(R.maxlen, (int)R.nzp[a + 1] - (int)R.nzp[a]);
          const int n_blk = std::abs(s->blk_local[k]);
          for (int q = 0; q < R.nnz; ++q) {
            R.nzt[q] = psd_closed_tab_entry(n_blk, le[z0 + q]);
            R.v[q] = lval[z0 + q];
            int rowpos = 0;
            while (rowpos + 1 <= nk && (int)R.nzp[rowpos + 1] <= q) ++rowpos;
            int mult = 0;
            for (int q2 = 0; q2 < q; ++q2) mult += le[z0 + q2] == le[z0 + q];
            R.rk[q] = (unsigned char)(rowpos | (mult << 3));
            maxmult = std::max(maxmult, mult + 1);
            if (mult > 31) ok = false;
          }
          R.nrounds = maxmult;
        }
      }
      if (ok && s->upa.in_update) {
        // cuadmm_update_A: the same records with the new rows of A, normA, D, dense factor and b, into the allocation of init in one copy
        // (headers, nk / nnz / rounds, depend on the pattern alone: the descriptors' aux words stay)
        if (s->closed.rec.n != recs.size()) { set_error("update_A: the closed-block records changed their number"); return CUADMM_ERR_INTERNAL; }
        if ((rc = s->closed.rec.upload(recs.data(), recs.size()))) return rc;
        s->upa.bytes += (double)(sizeof(ClosedRec) * recs.size());
        s->closed.active = true;
      } else if (ok) {
        if ((rc = s->closed.rec.from(recs)) || (rc = s->closed.cl_out.alloc(16 * recs.size())) ||
            (rc = s->closed.partials2.alloc(2 * (size_t)s->plan.fused_blocks() + 2)))
          return rc;
        CUADMM_HIP_TRY(hipMemset(s->closed.cl_out.p, 0, sizeof(double) * 16 * recs.size()));
        {   // the records' headers travel with the block descriptors (one dependent load less in every kernel that reads them)
          std::vector<int> aux(nb, 0);
          for (size_t k = 0; k < nb; ++k)
            if (slot_of[k] >= 0) { const ClosedRec& R = recs[(size_t)slot_of[k]]; aux[k] = closed_hdr_pack(R.nk, R.nnz, R.nrounds, R.maxlen); }
          if ((rc = s->plan.set_desc_aux(aux))) return rc;
        }
        s->closed.active = true;
        s->closed.out_dirty = true;
        if (s->verbose) printf(" closed blocks: each block solves for its own multipliers (<= %d rows) inside the projection kernel\n", kClosedMaxRows);
      }
    }
  }
  return rc;
}

static int init_residuals(Solver* s, bool y_resident);
// stage: device copies of b / normA for the device-side scalars, mapped result buffers, initial residuals (solver.cu:195-228)
static int init_finish(Solver* s, const InitIn& in, InitCtx& c) {
  CUADMM_INIT_STAGE_PROLOGUE
  if (s->dev_scalars || s->dev_solve) {
    if ((rc = s->b_d.alloc(std::max(m, 1))) || (rc = s->normA_d.alloc(std::max(m, 1)))) return rc;
    if ((rc = s->b_d.upload(s->b_p.data(), (size_t)m)) || (rc = s->normA_d.upload(s->normA_p.data(), (size_t)m))) return rc;
    void* dp = nullptr;
    if (s->sw.mapped_out && hipHostGetDevicePointer(&dp, s->h_scal.p, 0) == hipSuccess && dp) s->h_scal_dev = static_cast<double*>(dp);
    else { hipError_t e = hipGetLastError(); (void)e; }
  }
  if (s->world <= 1 && !s->force_comm && !s->dev_scalars && !s->dev_solve && s->sw.mapped_out) {
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, s->h_out.p, 0) == hipSuccess && dp) { s->out_w = static_cast<double*>(dp); s->out_mapped = true; }
    else { hipError_t e = hipGetLastError(); (void)e; }
  }

  return init_residuals(s, false);
}

// last stage of init, and of cuadmm_update_bC: initial A X, A (S - C) and residual scalars (solver.cu:195-228) from the scaled X, y, S.
// y_resident: y_d already holds y (the update rescaled it there), nothing to upload
static int init_residuals(Solver* s, bool y_resident) {
  const int m = s->m;
  const long long L = s->L;
  int rc = CUADMM_OK;
  if (!y_resident && (rc = s->upload_y(true))) return rc;
  if ((rc = s->launch_aty(false))) return rc;                               // Rd1 = At*y - C
  if ((rc = launch_post(2, L, s->Xproj.p, s->Rd1.p, s->C.p, s->X.p, s->S.p, 1.0, 0.0, s->partials.p,
                        s->out_w + (size_t)m, s->st)))                      // Rd = Rd1 + S, sums (X untouched)
    return rc;
  if ((rc = s->launch_spmv(true, true))) return rc;
  if ((rc = s->fetch_out(0, 2 * (size_t)m + 2))) return rc;
  {
    double nr = 0, bty = 0;
    s->refresh_Rp();
    for (int i = 0; i < m && !s->dev_solve; ++i) {
      double ro = s->normA_p[i] * s->Rp_p[i] * s->bscale;
      nr += ro * ro;
      bty += s->b_p[i] * s->y_p[i];
    }
    {
      double v[4] = {nr, bty, s->h_out.p[(size_t)m], s->h_out.p[(size_t)m + 1]};
      if (s->dev_scalars || s->dev_solve) { for (int q = 0; q < 4; ++q) v[q] = s->h_scal.p[q]; }   // formed (and summed over ranks) on the device
      else if ((rc = s->allreduce_scalars(v, 4))) return rc;
      nr = v[0]; bty = v[1]; s->h_out.p[(size_t)m] = v[2]; s->h_out.p[(size_t)m + 1] = v[3];
    }
    s->set_residual_scalars(nr, bty);
  }
  return rc;
}

#undef CUADMM_INIT_STAGE_PROLOGUE
}  // namespace

extern "C" {

const char* cuadmm_last_error(void) { return get_error(); }
const char* cuadmm_version(void) { return "cuadmm_amd 0.1 (gfx950)"; }
int cuadmm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int cuadmm_create(cuadmm_solver** out) {
  if (!out) { set_error("create: null"); return CUADMM_ERR_INVALID; }
  *out = new cuadmm_solver();
  return CUADMM_OK;
}
void cuadmm_destroy(cuadmm_solver* s) {
  if (s && s->group) { duo_group_destroy(s->group); s->group = nullptr; }
  delete s;
}

int cuadmm_set_option(cuadmm_solver* s, const char* key, double value) {
  if (!s || !key) { set_error("set_option: null"); return CUADMM_ERR_INVALID; }
  std::string k(key);
  s->option_log.emplace_back(k, value);
  if (k == "device") s->device = (int)value;
  else if (k == "verbose") s->verbose = (int)value;
  else if (k == "rank") s->rank = (int)value;
  else if (k == "world") s->world = (int)value;
  else if (k == "profile") s->profile = (int)value;
  else if (k == "force_comm") s->force_comm = (int)value;   // call the collective hook even when world == 1 (testing)
  else if (k == "eig_rank") s->eig_rank = (int)value;
  else if (k == "eig_rank_begin_iter") s->eig_rank_begin_iter = (int)value;
  else if (k == "eig_rank_maxfeas") s->eig_rank_maxfeas = value;
  else if (k == "psd_steps") s->psd_steps = (int)value;       // record the sign kernels' step count per block (cuadmm_get_psd_steps)
  else if (k == "batch") s->bt.max_iters = std::max(0, std::min(256, (int)value));   // iterations per launch, closed blocks (0 / 1: off)
  else if (k == "fuse") s->sw.fuse = (int)value;
  else if (k == "fuse_rows") s->sw.fuse_rows = (int)value;
  else if (k == "fuse_solve") s->sw.fuse_solve = (int)value;
  else if (k == "host_solve") s->sw.host_solve = (int)value;
  else if (k == "host_scalars") s->sw.host_scalars = (int)value;
  else if (k == "tail_k") s->sw.tail_k = (int)value;
  else if (k == "local_constraints") s->sw.local_constraints = (int)value;
  else if (k == "mapped_out") s->sw.mapped_out = (int)value;
  else if (k == "lpt") s->sw.lpt = (int)value;
  else if (k == "aty_post2") s->sw.aty_post2 = (int)value;
  else if (k == "lead_stream") s->sw.lead_stream = (int)value;
  else if (k == "lead_debug") s->sw.lead_debug = (int)value;
  else if (k == "lead_tops") s->sw.lead_tops = (int)value;
  else if (k == "lead_small_kb") s->sw.lead_small_kb = (int)value;
  else if (k == "l21_device") s->sw.l21_device = (int)value;
  else if (k == "tail_one_pass") s->sw.tail_one_pass = (int)value;
  else if (k == "tail_shard") s->sw.tail_shard = (int)value;
  else if (k == "tail_refine") s->sw.tail_refine = (int)value;
  else if (k == "tail_pivot") s->sw.tail_pivot = (int)value;
  else if (k == "tail_max_k") s->sw.tail_max_k = (int)value;
  else if (k == "solve_next") s->sw.solve_next = (int)value;
  else if (k == "debug_eig") s->sw.debug_eig = (int)value;
  else if (s->plan.opt.set(k, value)) {}                      // "psd_*": the projection planner's switches (psd_options.h)
  else if (k == "batch_mixed") s->bt.allow_mixed = value != 0;
  else if (k == "lazy_unscale") s->lazy_unscale = (int)value;            // 0: unscale X, y, S at the end of every solve
  else if (k == "psd_hint") s->opt_hint = (int)value;                    // schedule warm start (before init)
  else if (k == "duo_cpu_eig_on_gpu") s->duo_cpu_eig_on_gpu = (int)value;
  else if (k == "duo_share_device") s->duo_share_device = (int)value;   // duo_init(device_num_requested = N) from one process: all N engines on this solver's device
  else if (k == "tiny_sign") s->opt_tiny_sign = (int)value;              // n <= 8 on the sign kernel (before init)
  else if (k == "duo_exchange") s->duo_exchange = (int)value;           // in-process group: -1 choose, 0 host-staged, 1 device-side exchange
  else if (k == "accel") {                                              // memory of the Anderson acceleration (0: off), before init
    if (!(value >= 0 && value <= kAccelMaxMem && value == std::floor(value))) {
      s->option_log.pop_back(); set_error("set_option: accel must be an integer from 0 (off) to %d", kAccelMaxMem); return CUADMM_ERR_INVALID;
    }
    s->aa.mem = (int)value;
  }
  else if (k == "accel_safeguard") s->aa.safeguard = value;             // a candidate is rejected when ||g|| grows by more than this factor (<= 0: always)
  else if (k == "accel_reg") s->aa.reg = value;                         // relative Tikhonov term of the least-squares solve
  else if (k == "infeas_check") {                                       // period of the infeasibility check (0: off), before init
    if (!(value == 0 || (value >= 2 && value <= 1e6 && value == std::floor(value)))) {
      s->option_log.pop_back(); set_error("set_option: infeas_check must be 0 (off) or an integer period from 2 to 1000000"); return CUADMM_ERR_INVALID;
    }
    if (s->initialised) { s->option_log.pop_back(); set_error("set_option: infeas_check is set before init"); return CUADMM_ERR_INVALID; }
    s->inf.period = (int)value;
  }
  else if (k == "infeas_tol") {
    if (!(value >= 0)) { s->option_log.pop_back(); set_error("set_option: infeas_tol must not be negative"); return CUADMM_ERR_INVALID; }
    s->inf.tol = value;
  }
  else if (k == "gap_check") {                                          // period of the certified-gap check (0: off), before init
    if (!(value == 0 || (value >= 2 && value <= 1e6 && value == std::floor(value)))) {
      s->option_log.pop_back(); set_error("set_option: gap_check must be 0 (off) or an integer period from 2 to 1000000"); return CUADMM_ERR_INVALID;
    }
    if (s->initialised) { s->option_log.pop_back(); set_error("set_option: gap_check is set before init"); return CUADMM_ERR_INVALID; }
    s->lb.period = (int)value;
  }
  else if (k == "gap_tol") {
    if (!(value >= 0)) { s->option_log.pop_back(); set_error("set_option: gap_tol must not be negative"); return CUADMM_ERR_INVALID; }
    s->lb.tol = value;
  }
  else if (k == "update_A_inject_fail") s->upa.inject_fail = (int)value;   // test hook
  else if (k == "duo_inject_fail") { s->duo_inject = (long long)value; if (s->group) duo_group_inject(s->group, s->duo_inject); }   // test hook
  else { s->option_log.pop_back(); set_error("set_option: unknown key '%s'", key); return CUADMM_ERR_INVALID; }
  // a group handle: every rank follows -- AFTER the key has been validated on the leader; a child that refuses leaves the option
  // out of the log (it is not replayed on later children) and the error with the caller
  if (s->group && !s->in_group_call && k != "device" && k != "rank" && k != "world" && k != "verbose" && k != "duo_inject_fail")
    for (int r = 1; r < duo_group_world(s->group); ++r) {
      int rc = cuadmm_set_option(duo_group_rank(s->group, r), key, value);
      if (rc) { s->option_log.pop_back(); return rc; }
    }
  return CUADMM_OK;
}

int cuadmm_set_allreduce(cuadmm_solver* s, cuadmm_allreduce_fn fn, void* user) {
  if (!s) { set_error("set_allreduce: null"); return CUADMM_ERR_INVALID; }
  s->allreduce = fn; s->allreduce_user = user;
  return CUADMM_OK;
}

int cuadmm_rccl_unique_id(char out128[128]) {
  if (!g_rccl.load()) { set_error("RCCL not loadable"); return CUADMM_ERR_COMM; }
  NcclUid id;
  if (g_rccl.GetUniqueId(&id)) { set_error("ncclGetUniqueId failed"); return CUADMM_ERR_COMM; }
  std::memcpy(out128, id.internal, 128);
  return CUADMM_OK;
}

int cuadmm_use_rccl(cuadmm_solver* s, const char unique_id128[128], int rank, int world) {
  if (!s || !unique_id128) { set_error("use_rccl: null"); return CUADMM_ERR_INVALID; }
  if (!g_rccl.load()) { set_error("RCCL not loadable"); return CUADMM_ERR_COMM; }
  int rc = check_device(s->device);
  if (rc) return rc;
  NcclUid id;
  std::memcpy(id.internal, unique_id128, 128);
  if (g_rccl.CommInitRank(&s->rccl_comm, world, id, rank)) { set_error("ncclCommInitRank failed"); return CUADMM_ERR_COMM; }
  s->rank = rank; s->world = world;
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// SDPSolver::init
// ------------------------------------------------------------------------------------------
int cuadmm_init(cuadmm_solver* s, int eig_stream_num_per_gpu, int cpu_eig_thread_num, int vec_len, int con_num,
                const int* At_cp, const int* At_ri, const double* At_vx, int At_nnz, const int* b_idx,
                const double* b_vals, int b_nnz, const int* C_idx, const double* C_vals, int C_nnz,
                const int* blk, int mat_num, const double* X0, const double* y0, const double* S0, double sig) {
  (void)eig_stream_num_per_gpu; (void)cpu_eig_thread_num;
  if (!s) { set_error("init: null solver"); return CUADMM_ERR_INVALID; }
  if (s->initialised) { set_error("init: solver already initialised (one init per object, as in the reference)"); return CUADMM_ERR_INVALID; }
  if (vec_len < 0 || con_num < 0 || At_nnz < 0 || b_nnz < 0 || C_nnz < 0 || mat_num < 0 || !At_cp || !blk ||
      (At_nnz > 0 && (!At_ri || !At_vx)) || (b_nnz > 0 && (!b_idx || !b_vals)) || (C_nnz > 0 && (!C_idx || !C_vals))) {
    set_error("init: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  if (s->world < 1 || s->rank < 0 || s->rank >= s->world) { set_error("init: bad rank/world %d/%d", s->rank, s->world); return CUADMM_ERR_INVALID; }
  if (s->aa.mem > 0 && (s->world > 1 || s->eig_rank > 0 || s->group || s->in_group_call)) {
    set_error("init: option accel works on one rank with the full projection (world = %d, eig_rank = %d%s): its Gram matrix is not all-reduced",
              s->world, s->eig_rank, (s->group || s->in_group_call) ? ", in-process group" : "");
    return CUADMM_ERR_INVALID;
  }
  if (s->inf.period > 0 && (s->world > 1 || s->eig_rank > 0 || s->group || s->in_group_call || s->aa.mem > 0)) {
    set_error("init: option infeas_check works on one rank with the full projection and the plain iteration (world = %d, eig_rank = %d, accel = %d%s): "
              "its sums are not all-reduced, and differences of accelerated iterates are not the sequence its certificates come from",
              s->world, s->eig_rank, s->aa.mem, (s->group || s->in_group_call) ? ", in-process group" : "");
    return CUADMM_ERR_INVALID;
  }
  if (s->lb.period > 0 && (s->world > 1 || s->eig_rank > 0 || s->group || s->in_group_call || s->aa.mem > 0 || s->inf.period > 0)) {
    set_error("init: option gap_check works on one rank with the full projection and the plain iteration, without another check behind it "
              "(world = %d, eig_rank = %d, accel = %d, infeas_check = %d%s): its sums are not all-reduced, and one check at a time keeps the solve's end defined",
              s->world, s->eig_rank, s->aa.mem, s->inf.period, (s->group || s->in_group_call) ? ", in-process group" : "");
    return CUADMM_ERR_INVALID;
  }
  if (s->lb.period > 0 && s->lb.R.empty()) {
    set_error("init: option gap_check needs trace bounds (cuadmm_set_trace_bounds before cuadmm_init): without them no lower bound exists");
    return CUADMM_ERR_INVALID;
  }
  if (!s->lb.R.empty() && (int)s->lb.R.size() != mat_num) {
    set_error("init: %d trace bounds were set, the problem has %d blocks", (int)s->lb.R.size(), mat_num);
    return CUADMM_ERR_INVALID;
  }
  long long Lchk = 0;
  for (int k = 0; k < mat_num; ++k) {
    if (blk[k] == 0) { set_error("init: block %d has size 0", k); return CUADMM_ERR_INVALID; }
    Lchk += blk_svec_len(blk[k]);                       // negative size = unconstrained block of -blk[k] variables
  }
  if (Lchk != vec_len) { set_error("init: vec_len %d does not match blk (sum n(n+1)/2 = %lld)", vec_len, Lchk); return CUADMM_ERR_INVALID; }
  if (At_cp[0] != 0 || At_cp[con_num] != At_nnz) { set_error("init: At column pointers inconsistent with At_nnz"); return CUADMM_ERR_INVALID; }
  for (int p = 0; p < At_nnz; ++p)
    if (At_ri[p] < 0 || At_ri[p] >= vec_len) { set_error("init: At row index %d out of range at %d", At_ri[p], p); return CUADMM_ERR_INVALID; }

  if (s->world > 1) cuadmm_host_pool_hint(s->world);       // the ranks of a job share the node's CPUs (before the pool's first use)
  if (s->world > 1 && !s->local_mode && s->sw.local_constraints) {
    // does every constraint live inside one rank's block range?
    std::vector<int> first;
    partition_blocks(blk, mat_num, s->world, first);
    std::vector<long long> svb((size_t)s->world + 1, 0);
    {
      long long off = 0;
      int r = 0;
      for (int k = 0; k <= mat_num; ++k) {
        while (r <= s->world && first[r] == k) svb[r++] = off;
        if (k < mat_num) off += blk_svec_len(blk[k]);
      }
    }
    std::vector<int> owner(con_num, 0);
    bool all_owned = true;
    for (int j = 0; j < con_num && all_owned; ++j) {
      if (At_cp[j] == At_cp[j + 1]) continue;                      // empty constraint: rank 0
      const int r = (int)(std::upper_bound(svb.begin(), svb.end(), (long long)At_ri[At_cp[j]]) - svb.begin()) - 1;
      for (int p = At_cp[j]; p < At_cp[j + 1]; ++p)
        if (At_ri[p] < svb[r] || At_ri[p] >= svb[r + 1]) { all_owned = false; break; }
      owner[j] = r;
    }
    if (all_owned) {
      const int me = s->rank;
      // global norms (solver.cu:169-191) from the full inputs every rank holds
      { int rc = check_sparse_idx("init", "b", b_idx, b_nnz, con_num); if (rc) return rc; }
      std::vector<double> norm_all((size_t)con_num);         // what a later cuadmm_update_bC divides the whole new b by
      for (int j = 0; j < con_num; ++j) norm_all[j] = cons_norm(At_vx, At_cp[j], At_cp[j + 1]);
      const double nb = sum_sq(b_vals, b_nnz), nc = sum_sq(C_vals, C_nnz), nb2 = sum_scaled_sq(b_idx, b_vals, b_nnz, norm_all.data());
      std::vector<int> cons, g2l(con_num, -1);
      for (int j = 0; j < con_num; ++j) if (owner[j] == me) { g2l[j] = (int)cons.size(); cons.push_back(j); }
      const long long lo = svb[me], hi = svb[me + 1];
      std::vector<int> lcp(cons.size() + 1, 0), lri, lbi, lCi;
      std::vector<double> lvx, lbv, lCv, ly0;
      for (size_t q = 0; q < cons.size(); ++q) {
        for (int p = At_cp[cons[q]]; p < At_cp[cons[q] + 1]; ++p) { lri.push_back((int)(At_ri[p] - lo)); lvx.push_back(At_vx[p]); }
        lcp[q + 1] = (int)lri.size();
      }
      for (int i = 0; i < b_nnz; ++i) if (g2l[b_idx[i]] >= 0) { lbi.push_back(g2l[b_idx[i]]); lbv.push_back(b_vals[i]); }
      for (int i = 0; i < C_nnz; ++i) {
        if (C_idx[i] < 0 || C_idx[i] >= vec_len) { set_error("init: C index %d out of range", C_idx[i]); return CUADMM_ERR_INVALID; }
        if (C_idx[i] >= lo && C_idx[i] < hi) { lCi.push_back((int)(C_idx[i] - lo)); lCv.push_back(C_vals[i]); }
      }
      if (y0) { ly0.resize(cons.size()); for (size_t q = 0; q < cons.size(); ++q) ly0[q] = y0[cons[q]]; }
      s->local_mode = true;
      s->comm_world = s->world; s->comm_rank = s->rank;
      s->m_full = con_num; s->cons_local = cons; s->cons_g2l = g2l; s->sv_off = lo; s->blk_off = first[me];
      s->L_caller = vec_len; s->nblk_caller = mat_num;
      s->ov_nb = nb; s->ov_nc = nc; s->ov_nb2 = nb2; s->normA_all = norm_all;
      s->upa.g_cp.assign(At_cp, At_cp + con_num + 1);
      s->upa.g_from.clear();
      for (size_t q = 0; q < cons.size(); ++q)
        for (int p = At_cp[cons[q]]; p < At_cp[cons[q] + 1]; ++p) s->upa.g_from.push_back(p);
      s->upa.bg_idx.assign(b_idx, b_idx + b_nnz); s->upa.bg_val.assign(b_vals, b_vals + b_nnz);
      s->world = 1; s->rank = 0;
      if (s->comm_rank != 0) s->verbose = 0;      // one console table per job
      int one = 0;
      return cuadmm_init(s, eig_stream_num_per_gpu, cpu_eig_thread_num, (int)(hi - lo), (int)cons.size(), lcp.data(),
                         lri.empty() ? &one : lri.data(), lvx.empty() ? nullptr : lvx.data(), (int)lri.size(),
                         lbi.empty() ? nullptr : lbi.data(), lbv.empty() ? nullptr : lbv.data(), (int)lbi.size(),
                         lCi.empty() ? nullptr : lCi.data(), lCv.empty() ? nullptr : lCv.data(), (int)lCi.size(),
                         blk + first[me], first[me + 1] - first[me], X0 ? X0 + lo : nullptr, y0 ? ly0.data() : nullptr,
                         S0 ? S0 + lo : nullptr, sig);
    }
  }

  InitIn in{vec_len, con_num, At_nnz, b_nnz, C_nnz, mat_num, At_cp, At_ri, b_idx, C_idx, blk, At_vx, b_vals, C_vals, X0, y0, S0, sig};
  InitCtx ctx;
  int rc;
  if ((rc = init_device(s, in, ctx)) || (rc = init_normalise(s, in, ctx)) || (rc = init_factor(s, in, ctx)) || (rc = init_plan(s, in, ctx)) ||
      (rc = init_matrices(s, in, ctx)) || (rc = init_vectors(s, in, ctx)) || (rc = init_solve_plan(s, in, ctx)) || (rc = init_closed(s, in, ctx)) ||
      (rc = s->reset_solve_state(s->t_init0)) ||       // (in front of the residual stage, as in the updates: it clears Rp)
      (rc = init_finish(s, in, ctx)))
    return rc;
  s->initialised = true;
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// SDPSolver::solve
// ------------------------------------------------------------------------------------------
int cuadmm_solve(cuadmm_solver* s, int max_iter, double stop_tol, int sig_update_threshold, int sig_update_stage_1,
                 int sig_update_stage_2, int switch_admm, double sigscale, int if_first) {
  if (!s || !s->initialised) { set_error("solve: solver not initialised"); return CUADMM_ERR_INVALID; }
  if (s->factor_bad) { set_error("solve: the last cuadmm_update_A could not factor the new A A^T; the solver needs a successful cuadmm_update_A first"); return CUADMM_ERR_FACTOR; }
  if (sig_update_stage_1 <= 0 || sig_update_stage_2 <= 0) { set_error("solve: sig_update stages must be positive"); return CUADMM_ERR_INVALID; }
  if (s->group && !s->in_group_call)      // the leader of an in-process group (duo_group.hip): every rank solves, on its own host thread
    return group_forward(s, [&](cuadmm_solver* q) {
      return cuadmm_solve(q, max_iter, stop_tol, sig_update_threshold, sig_update_stage_1, sig_update_stage_2, switch_admm, sigscale, if_first);
    });
  int rc = check_device(s->device);
  if (rc) return rc;
  s->y_early = false;                       // (a solve that ended in an error may have left it set)
  // the dense tail of the replicated y-solve: split by rows over the ranks of a sharded engine (tail_solve.h)
  if (s->tail.k > 0) {
    const bool shard = s->world > 1 && !s->local_mode && s->sw.tail_shard != 0;
    s->tail.shard_rank = shard ? s->rank : 0;
    s->tail.shard_world = shard ? s->world : 1;
    s->tail.reduce_user = s;
    s->tail.reduce_fn = [](void* user, double* buf, size_t count, hipStream_t) -> int { return static_cast<cuadmm_solver*>(user)->comm_allreduce(buf, count); };
  }
  const int m = s->m;
  const long long L = s->L;
  const bool verbose = s->verbose && s->rank == 0;
  bool breakyes = false;
  std::string final_msg;
  s->info_iter_num = 0;

  if (verbose) {
    printf("\n -------------------------------------------------------------------------------");
    printf("\n                                    cuADMM");
    printf("\n -------------------------------------------------------------------------------");
    printf("\n norm of C = %2.1e, norm of b = %2.1e\n", s->norm_Corg, s->norm_borg);
  }

  if (if_first && s->pending_unscale && (rc = s->materialise())) return rc;   // the reference's X, y, S are unscaled after a solve
  if (!if_first && s->pending_unscale) {
    // the previous solve left X, y, S scaled and [A X | A (S - C)], Rp as its last iteration formed them: nothing to redo
    s->pending_unscale = false;
  } else if (!if_first) {   // solver.cu:385-409: X,y,S currently hold UNSCALED values
    if ((rc = s->sync_y_host())) return rc;
    for (int i = 0; i < m; ++i) s->y_p[i] = (s->y_p[i] * s->normA_p[i]) * (1 / s->Cscale);
    if (s->dev_solve && (rc = s->upload_y(true))) return rc;
    if ((rc = launch_scale(s->X.p, L, 1 / s->bscale, s->st))) return rc;
    if ((rc = launch_scale(s->S.p, L, 1 / s->Cscale, s->st))) return rc;
    if ((rc = s->launch_spmv(true, true))) return rc;
    if ((rc = s->fetch_out(0, 2 * (size_t)m + 2))) return rc;
    s->refresh_Rp();
  }

  if (verbose) {
    std::cout << std::endl << "  it. | p infeas d infeas | primal obj.   dual obj. rel. gap |  time |   sigma | " << std::endl;
    std::cout << " -------------------------------------------------------------------------------" << std::endl;
  }

  if ((rc = s->batch_agree())) return rc;
  if (s->accel_on() && (rc = s->accel_begin_solve())) return rc;
  s->solve_status = 0;
  if (s->infeas_on() && (rc = s->infeas_begin_solve())) return rc;
  s->lb_reset();
  s->lb.ms = 0;
  if (s->gap_on() && (rc = s->lb_prepare())) return rc;
  const bool lpt_enabled = s->sw.lpt != 0;
  long long& lpt_ev = s->lpt_next;             // counts iterations over all solve calls of this solver
  if (!lpt_enabled) lpt_ev = 0;
  // iteration i may change sigma in its step 5 (by reference: the switch to ADMM halves sig_update_stage_2 mid-solve)
  const auto sig_may_change_at = [&](int i) {
    return (i <= sig_update_threshold && i % sig_update_stage_1 == 1) || (i > sig_update_threshold && i % sig_update_stage_2 == 1);
  };
  for (int iter = 1; iter <= max_iter + 1; ++iter) {
    // ---- Step 0 (solver.cu:419-467)
    if (std::max(s->maxfeas, s->relgap) < stop_tol) { breakyes = true; final_msg = "Solver ended: converged."; }
    if (iter > max_iter) { breakyes = true; final_msg = "Solver ended: maximum iteration reached"; }
    if (s->solve_status == 5) {           // the certified gap behind the previous iteration (lb_step)
      breakyes = true;
      char msg[160];
      snprintf(msg, sizeof msg, "Solver ended: certified gap %.3e (lower bound %.10e at iteration %d)", s->lb.last_g, s->lb.last_lb, s->solve_status_iter);
      final_msg = msg;
    } else if (s->solve_status >= 3) {    // a certificate behind the previous iteration (infeas_step)
      breakyes = true;
      char msg[128];
      snprintf(msg, sizeof msg, "Solver ended: %s infeasible (certificate at iteration %d)", s->solve_status == 3 ? "primal" : "dual", s->solve_status_iter);
      final_msg = msg;
    } else if (breakyes) {
      s->solve_status = iter > max_iter ? 2 : 1;
      s->solve_status_iter = iter - 1;
    }
    const double seconds = wall_s() - s->t_init0;
    if (verbose && (breakyes || (iter <= 200 && iter % 50 == 1) || (iter > 200 && iter % 100 == 1))) {
      printf(" %4d | %3.2e %3.2e | %- 5.4e %- 5.4e %3.2e | %5.1f | %2.1e |", iter - 1, s->errRp, s->errRd, s->pobj,
             s->dobj, s->relgap, seconds, s->sig);
      std::cout << std::endl;
    }
    if (breakyes) {
      if (verbose) {
        printf("\n -------------------------------------------------------------------------------\n\n");
        std::cout << final_msg << std::endl;
        printf("\n primal infeasibility = %2.1e \n dual   infeasibility = %2.1e \n relative gap         = %2.1e", s->errRp,
               s->errRd, s->relgap);
        printf("\n primal objective = %- 9.8e \n dual   objective = %- 9.8e", s->pobj, s->dobj);
        printf("\n\n time per iteration = %2.4fs \n total time         = %2.1fs", seconds / iter, seconds);
        printf("\n -------------------------------------------------------------------------------\n\n");
      }
      s->total_time = wall_s() - s->t_init0;
    }

    // the device is ahead of the host schedule by the unconsumed iterations of a batch: back to the accepted state
    if (breakyes && s->bt.len > 0 && (rc = s->batch_rollback(s->bt.pos))) return rc;

    // ---- Step 1 (solver.cu:478-500): y = (AA^T)^-1 (Rp/sig - A(S-C)); with closed blocks the fused projection of this
    // iteration solves it (not on the last pass through the loop, which stops before the projection)
    if (s->y_early) s->y_early = false;       // enqueued at the end of the previous iteration (fetch_out, solve_next)
    else if (s->solve_status == 5) {}         // the bound was formed at the y the solve returns: no further y-solve behind the verdict
    else if (s->bt.len == 0 && (rc = s->host_solve(s->fuse && !breakyes))) return rc;

    if (breakyes) {   // solver.cu:567-576
      if (iter > switch_admm && s->have_best && s->solve_status < 3) {   // (a certificate describes the last iterate: no restore)
        CUADMM_HIP_TRY(hipMemcpyAsync(s->X.p, s->X_best.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, s->st));
        CUADMM_HIP_TRY(hipMemcpyAsync(s->S.p, s->S_best.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, s->st));
        CUADMM_HIP_TRY(hipStreamSynchronize(s->st));
        if (s->dev_solve) CUADMM_HIP_TRY(hipMemcpy(s->y_d.p, s->y_best_d.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice));
        else std::copy(s->y_best_p.begin(), s->y_best_p.end(), s->y_p.begin());   // in place: y_p's storage is page-locked
        if (verbose) printf("best max KKT residual after switch  = %2.1e \n", s->best_KKT);
      }
      break;
    }

    // ---- Step 2 (solver.cu:514-656).  The host-side decisions of this iteration (tau, snapshot) depend only on the previous
    // iteration's scalars, so they are taken first: the fused projection needs to know which post step follows it.
    double tau = (iter < switch_admm) ? 1.95 : 1.618;                    // solver.cu:747-754
    if (s->errRd < stop_tol) tau = std::max(1.618, tau / 1.1);

    // does this iteration snapshot the iterate between the S update and the X update?
    bool snapshot = false;
    if (iter == switch_admm) {                                           // solver.cu:681-690
      if (verbose) std::cout << " switching to normal ADMM!" << std::endl;
      sig_update_stage_2 = sig_update_stage_2 / 2;
      if (sig_update_stage_2 < 1) sig_update_stage_2 = 1;
      sigscale = sigscale * 1.23;
      s->sgs_KKT = std::max(s->maxfeas, s->relgap);
      s->best_KKT = s->sgs_KKT;
      snapshot = true;
    } else if (iter > switch_admm && s->have_best && !s->aa.pending && s->best_KKT > std::max(s->maxfeas, s->relgap)) {
      // (not in an iteration that started from a candidate of the acceleration: X, y, S there are not the iterate the scalars describe)
      s->best_KKT = std::max(s->maxfeas, s->relgap);                     // solver.cu:732-741
      snapshot = true;
    }

    const int post_mode_after_proj = (iter < switch_admm || snapshot) ? 1 : 0;
    // ---- several iterations in one launch (SignFuse::iters): ADMM phase without best-iterate bookkeeping, every block closed.
    // A batch ends at the next iteration that may change sigma; tau changes only through the errRd < stop_tol rule, checked
    // below on every consumed iteration.
    if (s->bt.len > 0 && tau != s->bt.tau) {
      // this iteration was run with the wrong step length: keep the consumed ones, continue one launch at a time
      if ((rc = s->batch_rollback(s->bt.pos))) return rc;
    }
    if (s->bt.len == 0 && iter > switch_admm && !s->have_best && !snapshot && s->can_batch()) {
      if ((rc = s->batch_alloc())) return rc;
      int K = std::min(std::min(s->bt.max_iters, s->bt.cap), max_iter - iter + 1);
      for (int j = 0; j < K; ++j) {          // the batch may END on a sigma-update iteration, not contain one
        if (sig_may_change_at(iter + j)) { K = j + 1; break; }
      }
      if (K >= 2) {
        // a batch can only be invalidated by the stopping test or the errRd < stop_tol rule for tau: no checkpoint without a tolerance
        s->bt.have_ck = stop_tol > 0.0;
        if (s->bt.have_ck && (rc = s->batch_copy(true))) return rc;
        s->bt.tau = tau; s->bt.sig = s->sig;
        // longest block first without a stall: the step counts are fetched behind one batch; the next one is launched in the new
        // order (the copy of the sorted descriptors is queued on the stream ahead of the launch; the host sort takes ~0.1 ms)
        const bool lpt_sorted_now = lpt_ev > 0 && s->steps_d.p && s->lpt_steps_ready;
        if (lpt_sorted_now) {
          if ((rc = s->plan.reorder_by_steps_async(s->steps_pin.p, s->st))) return rc;
          s->lpt_steps_ready = false;
          lpt_ev *= 8;
        }
        if ((rc = s->launch_fused_step(0, tau, K))) return rc;
        if (lpt_ev > 0 && s->steps_d.p && !lpt_sorted_now) {
          if (s->lpt_iters + K >= lpt_ev) {
            if (!s->steps_pin.p && (rc = s->steps_pin.alloc(s->steps_d.n))) return rc;
            CUADMM_HIP_TRY(hipMemcpyAsync(s->steps_pin.p, s->steps_d.p, sizeof(int) * s->steps_d.n, hipMemcpyDeviceToHost, s->st));
            s->lpt_steps_ready = true;     // valid once the stream has been synchronised (below)
          }
        }
        CUADMM_HIP_TRY(hipStreamSynchronize(s->st));
        s->prof_collect();
        s->bt.len = K; s->bt.pos = 0;
      }
    }
    const bool from_batch = s->bt.len > 0;
    // the next iteration's y-solve may follow this iteration's last kernel at once (fetch_out, solve_next): the whole solve is on the
    // device and belongs to the engine (not to a closed block's kernel), sigma does not change in this iteration's step 5, nothing of a
    // batch is pending, and the per-class event timers (profile = 1) are off -- they are collected at the wait, before that solve ends
    const bool sig_may_change = sig_may_change_at(iter);
    const bool solve_next_ok = s->sw.solve_next != 0 && !s->accel_on() && !s->infeas_on() && !s->gap_on() && s->dev_solve && !from_batch && !sig_may_change && !(s->fuse && s->closed.active) && s->profile != 1;
    if (from_batch) {
      // consumed below (Step 5) from bt.h
    } else if ((rc = s->upload_y())) return rc;
    if (from_batch) {
    } else if (s->fuse) {
      if ((rc = s->launch_fused_step(post_mode_after_proj, tau))) return rc;
    } else {
      if ((rc = s->launch_aty(true))) return rc;
      s->plan.rank_active = s->eig_rank > 0 && (iter >= s->eig_rank_begin_iter || s->maxfeas < s->eig_rank_maxfeas);   // duo_solver.cu:844
      if ((rc = s->launch_project())) return rc;
      const char* const debug_eig_dir = s->sw.debug_eig ? getenv("CUADMM_DEBUG_EIG") : nullptr;
      if (debug_eig_dir) {   // developer aid (option debug_eig + CUADMM_DEBUG_EIG=<dir>): dump the projection input when a block hits the QL cap
        int f = s->plan.fail_count(s->st);
        if (f != s->eig_fail_total) {
          fprintf(stderr, "[cuadmm debug] iter %d: QL cap hits %d -> %d\n", iter, s->eig_fail_total, f);
          std::vector<double> h((size_t)L);
          if (staged_d2h(h.data(), s->Xb.p, sizeof(double) * (size_t)L, s->st) == CUADMM_OK) {
            char fn[256];
            snprintf(fn, sizeof fn, "%s/xb_fail_iter%d.bin", debug_eig_dir, iter);
            if (FILE* fp = fopen(fn, "wb")) { fwrite(h.data(), sizeof(double), (size_t)L, fp); fclose(fp); }
          }
          s->eig_fail_total = f;
        }
      }
    }

    if (from_batch) {
    } else if (iter < switch_admm) {
      // sGS half step: S^{k+1}, second solve with it, Rd1 from the new y (solver.cu:693-729)
      if (!s->fuse && (rc = s->launch_post_mode(1, tau))) return rc;     // fused: done with the projection
      if ((rc = s->launch_spmv(false, true, s->fuse))) return rc;
      if ((rc = s->fetch_out((size_t)m + 2, (size_t)m))) return rc;
      if ((rc = s->host_solve())) return rc;
      if ((rc = s->upload_y())) return rc;
      if (s->At_long.nlong == 0 && s->sw.aty_post2) {   // one pass, Rd1 not stored (vec_kernels.hip)
        s->prof_begin(K_POST);
        rc = launch_aty_post2(L, s->At_rp.p, s->At_ci.p, s->At_v.p, s->y_d.p, s->C.p, s->S.p, s->X.p, tau * s->sig, s->partials.p,
                              s->out_w + (size_t)m, s->st);
        s->prof_end(K_POST, 40.0 * (double)L);
        if (rc) return rc;
      } else {
        if ((rc = s->launch_aty(false))) return rc;
        if ((rc = s->launch_post_mode(2, tau))) return rc;
      }
      if ((rc = s->launch_spmv(true, false))) return rc;
      if ((rc = s->fetch_out(0, (size_t)m + 2, solve_next_ok))) return rc;   // [A*X | sums]; A*(S-C) unchanged since the half step
    } else {
      if (snapshot) {
        if (!s->X_best.p && L > 0) { if ((rc = s->X_best.alloc(L)) || (rc = s->S_best.alloc(L))) return rc; }
        if (!s->fuse && (rc = s->launch_post_mode(1, tau))) return rc;
        s->prof_begin(K_COPY);
        CUADMM_HIP_TRY(hipMemcpyAsync(s->X_best.p, s->X.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, s->st));
        CUADMM_HIP_TRY(hipMemcpyAsync(s->S_best.p, s->S.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, s->st));
        s->prof_end(K_COPY, 32.0 * (double)L);
        if (s->dev_solve) {
          if (!s->y_best_d.p && (rc = s->y_best_d.alloc(std::max(m, 1)))) return rc;
          CUADMM_HIP_TRY(hipMemcpyAsync(s->y_best_d.p, s->y_d.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, s->st));
        } else {
          s->y_best_p = s->y_p;
        }
        s->have_best = true;
        if ((rc = s->launch_post_mode(2, tau))) return rc;
      } else if (!s->fuse) {
        if ((rc = s->launch_post_mode(0, tau))) return rc;
      }
      if ((rc = s->launch_spmv(true, true, s->fuse && !snapshot))) return rc;
      if ((rc = s->fetch_out(0, 2 * (size_t)m + 2, solve_next_ok))) return rc;
    }

    // ---- Step 5 (solver.cu:764-799)
    const double sig_of_iter = s->sig;
    {
      double t0 = wall_s();
      double nr = 0, bty = 0;
      const double* ax = s->h_out.p;
      double part[2 * kHostChunks] = {0};
      if (!s->dev_solve) host_ranges(m, [&](int c, int lo, int hi) {
        double a = 0, b = 0;
        for (int i = lo; i < hi; ++i) {
          const double rp = -ax[i] + s->b_p[i];
          s->Rp_p[i] = rp;
          const double ro = s->normA_p[i] * rp * s->bscale;
          a += ro * ro;
          b += s->b_p[i] * s->y_p[i];
        }
        part[2 * c] = a; part[2 * c + 1] = b;
      });
      for (int c = 0; c < kHostChunks; ++c) { nr += part[2 * c]; bty += part[2 * c + 1]; }
      {
        double v[4] = {nr, bty, s->h_out.p[(size_t)m], s->h_out.p[(size_t)m + 1]};
        if (from_batch) {
          for (int q = 0; q < 4; ++q) v[q] = s->bt.h.p[4 * (size_t)s->bt.pos + q];
          if (++s->bt.pos == s->bt.len) s->bt.len = s->bt.pos = 0;
        } else if (s->dev_scalars || s->dev_solve) { for (int q = 0; q < 4; ++q) v[q] = s->h_scal.p[q]; }   // formed (and summed over ranks) on the device
        else if ((rc = s->allreduce_scalars(v, 4))) return rc;
        nr = v[0]; bty = v[1]; s->h_out.p[(size_t)m] = v[2]; s->h_out.p[(size_t)m + 1] = v[3];
        // a lost row exchange of the four-workgroups-per-row tail kernel leaves NaN in y and with it in these sums: stop NOW (not at
        // max_iter), report once, and leave the handle on the two-GEMV path (TailSolve::take_failure)
        if (s->tail.d_fail && !(std::fabs(nr) <= 1.7976931348623157e308 && std::fabs(bty) <= 1.7976931348623157e308)) {
          const int tf = s->tail.take_failure(s->st);
          if (tf != 0) {
            set_error("solve: the dense tail of the A*A^T solve lost %d row exchanges at iteration %d (workgroups of a row not co-resident for seconds): "
                      "y is not valid; the handle now uses the two-pass tail kernels", tf, iter);
            return CUADMM_ERR_FACTOR;
          }
        }
      }
      s->set_residual_scalars(nr, bty);
      s->feasratio = s->ratioconst * s->errRp / s->errRd;
      if (s->feasratio < 1) s->prim_win += 1; else s->dual_win += 1;
      if (sig_may_change) {
        if (s->prim_win > 1.2 * s->dual_win) { s->prim_win = 0; s->sig = std::min(s->sigmax, s->sig * sigscale); }
        else if (s->dual_win > 1.2 * s->prim_win) { s->dual_win = 0; s->sig = std::max(s->sigmin, s->sig / sigscale); }
      }
      s->prof_host(K_HOST, wall_s() - t0);
    }
    s->info[CUADMM_INFO_POBJ].push_back(s->pobj); s->info[CUADMM_INFO_DOBJ].push_back(s->dobj);
    s->info[CUADMM_INFO_ERRRP].push_back(s->errRp); s->info[CUADMM_INFO_ERRRD].push_back(s->errRd);
    s->info[CUADMM_INFO_RELGAP].push_back(s->relgap); s->info[CUADMM_INFO_SIG].push_back(s->sig);
    s->info[CUADMM_INFO_BSCALE].push_back(s->bscale); s->info[CUADMM_INFO_CSCALE].push_back(s->Cscale);
    s->info_iter_num++;
    // longest block first (PsdPlan::reorder_by_steps): at iterations 3, 24, 192, ... of this solve the stream is idle here
    if (s->fuse && lpt_ev > 0) ++s->lpt_iters;
    if (s->fuse && lpt_ev > 0 && s->lpt_iters >= lpt_ev && s->bt.len == 0 && s->steps_d.p && !s->can_batch()) {
      s->steps_h.resize(s->steps_d.n);
      if ((rc = staged_d2h(s->steps_h.data(), s->steps_d.p, sizeof(int) * s->steps_d.n, s->st))) return rc;
      if ((rc = s->plan.reorder_by_steps(s->steps_h.data(), s->st))) return rc;
      lpt_ev *= 8;
    }
    // ---- acceleration: behind the iteration, on every path (the scalars above are those of the plain iterate f_k)
    if (s->accel_on()) {
      if ((rc = s->accel_step(iter, max_iter, stop_tol, switch_admm, tau, s->sig != sig_of_iter, sig_may_change_at(iter + 1)))) return rc;
    }
    // ---- infeasibility check: on the state at the end of the iteration, after the sigma update
    if (s->infeas_on() && iter % s->inf.period == 0 && (rc = s->infeas_step(iter, stop_tol))) return rc;
    // ---- certified-gap check: the lower bound at this iteration's y against this iteration's pobj
    if (s->gap_on() && iter % s->lb.period == 0 && (rc = s->lb_step(iter, stop_tol))) return rc;
  }

  // unscale (solver.cu:814-816) -- deferred until somebody reads or replaces X, y, S (materialise): a following
  // solve(if_first = false) continues from the scaled state.  With owned constraints over several ranks the y gather is a
  // collective, so there it happens here, where every rank is.
  s->pending_unscale = true;
  if (s->lazy_unscale == 0 || (s->local_mode && s->comm_world > 1)) { if ((rc = s->materialise())) return rc; }
  if (s->tail.k > 0) {
    const int tf = s->tail.take_failure(s->st);
    if (tf != 0) { set_error("solve: the dense tail of the A*A^T solve lost %d row exchanges (workgroups of a row not co-resident for seconds): y is not valid", tf); return CUADMM_ERR_FACTOR; }
  }
  s->eig_fail_total = s->plan.fail_count(s->st);
  if (s->eig_fail_total > 0) {
    set_error("solve: %d block projections hit the QL sweep cap", s->eig_fail_total);
    return CUADMM_ERR_EIG;
  }
  return CUADMM_OK;
}

// per-solve bookkeeping as init leaves it, in front of the residual stage (profile counters, plans, the blocks' launch order stay)
int cuadmm_solver::reset_solve_state(double t_begin) {
  for (auto& a : info) a.clear();
  info_iter_num = 0;
  t_init0 = t_begin; total_time = 0;
  best_KKT = 0; sgs_KKT = 0; have_best = false; eig_fail_total = 0;
  prim_win = 0; dual_win = 0; feasratio = 0; ratioconst = 1e0; sigmax = 1e3; sigmin = 1e-3;
  y_early = false; stats_fused = false;
  bt.len = bt.pos = 0; bt.have_ck = false;
  closed.iters_done = 0; closed.out_dirty = true;
  infeas_reset();
  lb_reset();
  plan.n_project = 0;
  if (hint_d.p) CUADMM_HIP_TRY(hipMemsetAsync(hint_d.p, 0, sizeof(int) * hint_d.n, st));     // the sign schedule's warm start
  if (closed.cl_out.p) CUADMM_HIP_TRY(hipMemsetAsync(closed.cl_out.p, 0, sizeof(double) * closed.cl_out.n, st));
  if (!dev_solve) std::fill(Rp_p.begin(), Rp_p.end(), 0.0);
  y_full.clear();
  return CUADMM_OK;
}

// y_d -> y_p after cuadmm_update_bC left the rescaled y on the device only
int cuadmm_solver::sync_y_host() {
  if (!y_host_stale) return CUADMM_OK;
  y_host_stale = false;
  if (m <= 0) return CUADMM_OK;
  int rc;
  if ((rc = check_device(device))) return rc;
  CUADMM_HIP_TRY(hipMemcpyAsync(h_y.p, y_d.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  std::memcpy(y_p.data(), h_y.p, sizeof(double) * (size_t)m);
  return CUADMM_OK;
}

int cuadmm_solver::materialise() {
  if (!pending_unscale) return sync_y_host();
  pending_unscale = false;
  y_host_stale = false;                 // y_d is copied down below
  int rc;
  if ((rc = check_device(device))) return rc;
  if ((rc = launch_scale(X.p, L, bscale, st))) return rc;
  if ((rc = launch_scale(S.p, L, Cscale, st))) return rc;
  if (dev_solve && m > 0) {
    if (y_registered) CUADMM_HIP_TRY(hipMemcpyAsync(y_p.data(), y_d.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
    else {   // never a runtime copy into pageable memory (staging.hip)
      CUADMM_HIP_TRY(hipMemcpyAsync(h_y.p, y_d.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
      CUADMM_HIP_TRY(hipStreamSynchronize(st));
      std::memcpy(y_p.data(), h_y.p, sizeof(double) * (size_t)m);
    }
  }
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  for (int i = 0; i < m; ++i) y_p[i] = y_p[i] / normA_p[i] * Cscale;
  if (local_mode) {   // y is replicated for the caller: gather the owned pieces once per solve
    y_full.assign((size_t)m_full, 0.0);
    for (int i = 0; i < m; ++i) y_full[cons_local[perm[i]]] = y_p[i];
    if (comm_world > 1 && m_full > 0) {
      if (!yfull_d.p && (rc = yfull_d.alloc((size_t)m_full))) return rc;
      if ((rc = staged_h2d(yfull_d.p, y_full.data(), sizeof(double) * (size_t)m_full, st))) return rc;
      if ((rc = comm_allreduce(yfull_d.p, (size_t)m_full))) return rc;
      if ((rc = staged_d2h(y_full.data(), yfull_d.p, sizeof(double) * (size_t)m_full, st))) return rc;
    }
  }
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// Acceleration (option "accel"): DESIGN.md, "Acceleration"
// ------------------------------------------------------------------------------------------
// start of every solve: buffers on first use, empty memory, u_0 = the state the first iteration starts from
int cuadmm_solver::accel_begin_solve() {
  int rc;
  if (!aa.fbuf.p) {
    aa.hs = (L + 1) & ~1LL;
    const size_t n2 = 2 * (size_t)aa.hs;
    if ((rc = aa.ring_dF.alloc(n2 * aa.mem)) || (rc = aa.ring_dG.alloc(n2 * aa.mem)) || (rc = aa.state[0].alloc(n2)) || (rc = aa.gbuf.alloc(n2)) ||
        (rc = aa.state[1].alloc(n2)) || (rc = aa.partials.alloc(kAccelPartials)) || (rc = aa.dots.alloc(kAccelDots)) || (rc = aa.h_dots.alloc(kAccelDots)) ||
        (rc = aa.fb_y.alloc(std::max(m, 1))) || (rc = aa.fb_out.alloc(2 * (size_t)m + 2)))
      return rc;
    aa.fbuf.p = aa.state[0].p; aa.ubuf.p = aa.state[1].p;
    // the pad element of an odd L is never read, but a column is copied whole nowhere either: zero once, for tidy dumps
    CUADMM_HIP_TRY(hipMemsetAsync(aa.ubuf.p, 0, sizeof(double) * n2, st));
    CUADMM_HIP_TRY(hipMemsetAsync(aa.fbuf.p, 0, sizeof(double) * n2, st));
    CUADMM_HIP_TRY(hipMemsetAsync(aa.gbuf.p, 0, sizeof(double) * n2, st));
    if (profile) for (auto& e : aa.ev) CUADMM_HIP_TRY(hipEventCreate(&e));
  }
  accel_clear();
  CUADMM_HIP_TRY(hipMemcpyAsync(aa.fbuf.p, X.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, st));
  CUADMM_HIP_TRY(hipMemcpyAsync(aa.fbuf.p + aa.hs, S.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, st));
  return CUADMM_OK;
}

// End of iteration `iter` (its scalars are recorded, sigma may have changed in its step 5).  X, S hold f_k = F(u_k).
int cuadmm_solver::accel_step(int iter, int max_iter, double stop_tol, int switch_admm, double tau, bool sig_changed, bool next_sig_may_change) {
  int rc;
  const size_t n2 = 2 * (size_t)aa.hs;
  const bool timed = profile != 0 && aa.ev[0];
  auto elapsed = [&](int a) { if (timed) aa.ms += event_ms(aa.ev[a], aa.ev[a + 1]); };   // after a synchronisation behind ev[a + 1]
  // the map changed under this iteration's feet (sigma in step 5): nothing held describes the new map.  (No candidate is ever
  // pending here: none is taken in front of an iteration that may change sigma.)
  if (sig_changed) {
    accel_clear();
    aa.restarts++;
    CUADMM_HIP_TRY(hipMemcpyAsync(aa.fbuf.p, X.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, st));
    CUADMM_HIP_TRY(hipMemcpyAsync(aa.fbuf.p + aa.hs, S.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, st));
    return CUADMM_OK;
  }
  // g_k, the new columns, f_k.  Behind a candidate u_k is ubuf and f_k goes there too, so that fbuf still holds the fallback.
  const bool was_pending = aa.pending;
  const bool have_col = aa.have_prev;
  const int slot = aa.head;
  double* const u = was_pending ? aa.ubuf.p : aa.fbuf.p;
  if (timed) CUADMM_HIP_TRY(hipEventRecord(aa.ev[0], st));
  if ((rc = launch_aa_push(L, aa.hs, u, X.p, S.p, sig, aa.fbuf.p, aa.gbuf.p, have_col ? 1 : 0, aa.gbuf.p, u, aa.ring_dF.p + (size_t)slot * n2,
                           aa.ring_dG.p + (size_t)slot * n2, aa.partials.p, aa.dots.p + 2 * kAccelMaxMem, st)))
    return rc;
  int cols_new = aa.cols;
  if (have_col) {
    cols_new = std::min(aa.cols + 1, aa.mem);
    if ((rc = launch_aa_gram(L, aa.hs, (long long)n2, cols_new, slot, aa.ring_dG.p, aa.gbuf.p, aa.partials.p, aa.dots.p, st))) return rc;
  }
  if (timed) CUADMM_HIP_TRY(hipEventRecord(aa.ev[1], st));
  CUADMM_HIP_TRY(hipMemcpyAsync(aa.h_dots.p, aa.dots.p, sizeof(double) * kAccelDots, hipMemcpyDeviceToHost, st));
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  elapsed(0);
  const double gnorm2 = aa.h_dots.p[2 * kAccelMaxMem];

  if (was_pending) {
    aa.pending = false;
    const bool reject = !(aa.safeguard > 0) || !(std::sqrt(gnorm2) <= aa.safeguard * std::sqrt(aa.gnorm2_prev));
    if (reject) {
      // back to f_k, bit for bit: X, S, y, the fetched vectors, the scalars of the stopping test.  The wasted iteration stays recorded.
      CUADMM_HIP_TRY(hipMemcpyAsync(X.p, aa.fbuf.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, st));
      CUADMM_HIP_TRY(hipMemcpyAsync(S.p, aa.fbuf.p + aa.hs, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, st));
      if (dev_solve) CUADMM_HIP_TRY(hipMemcpyAsync(y_d.p, aa.fb_y.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, st));
      else { std::copy(aa.h_fb_y.begin(), aa.h_fb_y.end(), y_p.begin()); std::copy(aa.h_fb_Rp.begin(), aa.h_fb_Rp.end(), Rp_p.begin()); }
      if (!out_mapped) CUADMM_HIP_TRY(hipMemcpyAsync(out_d.p, aa.fb_out.p, sizeof(double) * (2 * (size_t)m + 2), hipMemcpyDeviceToDevice, st));
      if (hint_d.p) CUADMM_HIP_TRY(hipMemcpyAsync(hint_d.p, aa.fb_hint.p, sizeof(int) * hint_d.n, hipMemcpyDeviceToDevice, st));
      plan.n_project = aa.fb_nproj; closed.iters_done = aa.fb_iters_done;
      CUADMM_HIP_TRY(hipStreamSynchronize(st));
      std::copy(aa.h_fb_out.begin(), aa.h_fb_out.end(), h_out.p);
      closed.out_dirty = true;
      errRp = aa.sc[0]; errRd = aa.sc[1]; maxfeas = aa.sc[2]; pobj = aa.sc[3]; dobj = aa.sc[4]; relgap = aa.sc[5]; feasratio = aa.sc[6];
      prim_win = aa.sc_win[0]; dual_win = aa.sc_win[1];
      accel_clear();
      aa.rejected++;
      return CUADMM_OK;
    }
    aa.accepted++;
    std::swap(aa.fbuf.p, aa.ubuf.p);      // f_k was written over the candidate
  }
  if (have_col) {
    // the Gram matrix by ring slot: row and column `slot` are the new column's
    for (int j = 0; j < cols_new; ++j) aa.G[slot][j] = aa.G[j][slot] = aa.h_dots.p[j];
    aa.cols = cols_new;
    aa.head = (slot + 1) % aa.mem;
  }
  aa.have_prev = true;

  // what the next iteration will be
  const int nx = iter + 1;
  double tau_next = (nx < switch_admm) ? 1.95 : 1.618;
  if (errRd < stop_tol) tau_next = std::max(1.618, tau_next / 1.1);
  if (tau_next != tau || nx == switch_admm) {     // another map from the next iteration on
    accel_clear();
    aa.restarts++;
    return CUADMM_OK;
  }
  // no candidate in front of the pass that stops (the result is a plain iterate), nor in front of a possible sigma update
  if (nx > max_iter || std::max(maxfeas, relgap) < stop_tol || next_sig_may_change || aa.cols < 2) return CUADMM_OK;

  double gram[kAccelMaxMem * kAccelMaxMem], rhs[kAccelMaxMem], gamma[kAccelMaxMem];
  for (int i = 0; i < aa.cols; ++i) {
    rhs[i] = aa.h_dots.p[cols_new + i];
    for (int j = 0; j < aa.cols; ++j) gram[i * aa.cols + j] = aa.G[i][j];
  }
  if (accel_solve_ls(gram, rhs, aa.cols, aa.reg, gamma) != CUADMM_OK) {     // degenerate columns: start the memory afresh
    accel_clear();
    aa.restarts++;
    return CUADMM_OK;
  }
  // the fallback beside fbuf: y, the fetched vectors, the host scalars
  if (dev_solve) CUADMM_HIP_TRY(hipMemcpyAsync(aa.fb_y.p, y_d.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, st));
  else { aa.h_fb_y = y_p; aa.h_fb_Rp = Rp_p; }
  if (!out_mapped) CUADMM_HIP_TRY(hipMemcpyAsync(aa.fb_out.p, out_d.p, sizeof(double) * (2 * (size_t)m + 2), hipMemcpyDeviceToDevice, st));
  if (hint_d.p) {
    if (!aa.fb_hint.p && (rc = aa.fb_hint.alloc(hint_d.n))) return rc;
    CUADMM_HIP_TRY(hipMemcpyAsync(aa.fb_hint.p, hint_d.p, sizeof(int) * hint_d.n, hipMemcpyDeviceToDevice, st));
  }
  aa.fb_nproj = plan.n_project; aa.fb_iters_done = closed.iters_done;
  aa.h_fb_out.assign(h_out.p, h_out.p + 2 * (size_t)m + 2);
  aa.sc[0] = errRp; aa.sc[1] = errRd; aa.sc[2] = maxfeas; aa.sc[3] = pobj; aa.sc[4] = dobj; aa.sc[5] = relgap; aa.sc[6] = feasratio;
  aa.sc_win[0] = prim_win; aa.sc_win[1] = dual_win;
  aa.gnorm2_prev = gnorm2;

  if (timed) CUADMM_HIP_TRY(hipEventRecord(aa.ev[2], st));
  if ((rc = launch_aa_combine(L, aa.hs, (long long)n2, aa.cols, aa.ring_dF.p, gamma, sig, X.p, S.p, aa.ubuf.p, st))) return rc;
  if (timed) CUADMM_HIP_TRY(hipEventRecord(aa.ev[3], st));
  // X and S were overwritten: [A X | sums | A (S - C)] and Rp again, as a continued solve forms them
  if ((rc = launch_spmv(true, true))) return rc;
  if ((rc = fetch_out(0, 2 * (size_t)m + 2))) return rc;
  refresh_Rp();
  elapsed(2);
  aa.pending = true;
  aa.taken++;
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// Infeasibility detection (option "infeas_check"): DESIGN.md, "Infeasibility certificates"
// ------------------------------------------------------------------------------------------
// Auxiliary projector (infeasibility check, lower bound)
int cuadmm_solver::AuxProj::ensure(cuadmm_solver& s) {
  int rc;
  if (!ev[1]) {
    if ((rc = in.alloc((size_t)s.L)) || (rc = out.alloc((size_t)s.L)) || (!s.b_d.p && (rc = bcopy.alloc((size_t)std::max(s.m, 1))))) return rc;
    for (auto& e : ev) CUADMM_HIP_TRY(hipEventCreate(&e));
  }
  if (bcopy.p && s.m > 0 && (rc = staged_h2d(bcopy.p, s.b_p.data(), sizeof(double) * (size_t)s.m, s.st))) return rc;
  return CUADMM_OK;
}
int cuadmm_solver::AuxProj::project(cuadmm_solver& s, const double* from, double* to) {
  if (!plan) {
    int rc;
    size_t free0 = 0, free1 = 0, total = 0;
    if (hipMemGetInfo(&free0, &total) != hipSuccess) { free0 = 0; (void)hipGetLastError(); }
    plan = new PsdPlan();
    plan->opt = s.plan.opt;
    plan->eig_rank = 0;
    if ((rc = plan->build(s.blk_local.data(), (int)s.blk_local.size()))) { delete plan; plan = nullptr; return rc; }
    if (hipMemGetInfo(&free1, &total) != hipSuccess) { free1 = free0; (void)hipGetLastError(); }
    plan_bytes = free0 > free1 ? (double)(free0 - free1) : 0.0;
  }
  projected = true;
  return plan->project(from, to, s.st);
}

// The y a report reads, in the engine's scaled space and the factor's order, in a vector of the report's own.  y_caller: the caller's,
// with the constants of materialise() inverted as cuadmm_init applies them.  Null: the y cuadmm_get_y would return -- behind a solve the
// iterate is held scaled and is copied as it lies (the deferred unscaling is not triggered: a following solve(if_first = false)
// continues from it bit for bit); otherwise y is in the caller's units, on the host, or on the device only where cuadmm_update_bC left
// the current one there.
int cuadmm_solver::stage_scaled_y(double* dst, const double* y_caller) {
  int rc;
  if (m <= 0) { CUADMM_HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double), st)); return CUADMM_OK; }
  if (!y_caller && pending_unscale && dev_solve) {
    CUADMM_HIP_TRY(hipMemcpyAsync(dst, y_d.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, st));
    return CUADMM_OK;
  }
  std::vector<double> ys(y_p);
  const double ics = 1 / Cscale;
  if (y_caller) for (int i = 0; i < m; ++i) ys[i] = (y_caller[perm[i]] * normA_p[i]) * ics;
  else if (!pending_unscale) {
    if (y_host_stale && (rc = staged_d2h(ys.data(), y_d.p, sizeof(double) * (size_t)m, st))) return rc;
    for (int i = 0; i < m; ++i) ys[i] = (ys[i] * normA_p[i]) * ics;
  }
  return staged_h2d(dst, ys.data(), sizeof(double) * (size_t)m, st);
}

// M = A'y - C by the iteration's kernel into the auxiliary projector's input vector (S^ = -Cscale M), and the slot sums of b'y
int cuadmm_solver::dual_slack(const double* y, double* by_part) {
  int rc;
  if ((rc = launch_aty_xb(false, L, At_rp.p, At_ci.p, At_v.p, y, C.p, X.p, 1.0, aux.in.p, nullptr, st, &At_long))) return rc;
  return launch_lb_dot(m, aux.b_dev(*this), y, by_part, st);
}

// start of every solve: buffers on first use, no snapshot
int cuadmm_solver::infeas_begin_solve() {
  int rc;
  if (!inf.xprev.p) {
    const size_t mm = (size_t)std::max(m, 1);
    if ((rc = inf.xprev.alloc(L)) || (rc = inf.yprev.alloc(mm)) || (rc = inf.dy.alloc(mm)) ||
        (rc = inf.adx.alloc(mm)) || (rc = inf.partials.alloc(kInfeasPartials)) || (rc = inf.stats_d.alloc(INF_NSTATS)) || (rc = inf.h_stats.alloc(INF_NSTATS)))
      return rc;
    long long off = 0;
    for (int n : blk_local) { if (n < 0) inf.free_rng.emplace_back(off, blk_svec_len(n)); off += blk_svec_len(n); }
  }
  if ((rc = aux.ensure(*this))) return rc;
  infeas_reset();
  inf.ms = 0;
  return CUADMM_OK;
}

// End of iteration `iter`, a multiple of the period.  y_d holds the y this iteration's A^T y kernel read (device y-solve: its result,
// host y-solve: the uploaded copy), in the factor's order; X the new X.  The first call of a solve only copies the snapshot.
int cuadmm_solver::infeas_step(int iter, double stop_tol) {
  int rc;
  if (std::max(maxfeas, relgap) < stop_tol) return CUADMM_OK;      // the loop is about to end as converged
  if (!inf.have_snap) {          // the first multiple of the period: the snapshot alone
    if (m > 0) CUADMM_HIP_TRY(hipMemcpyAsync(inf.yprev.p, y_d.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, st));
    CUADMM_HIP_TRY(hipMemcpyAsync(inf.xprev.p, X.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, st));
    inf.have_snap = true;
    return CUADMM_OK;
  }
  double* const dbuf = aux.in.p;      // a difference, the input of a projection
  double* const pbuf = aux.out.p;     // its PSD part
  if ((rc = aux.begin(st))) return rc;
  // d = cur - prev and prev <- cur in one pass each; the X difference is written negated: it is the input of P+(-dX), and the norm
  // of A dX does not see the sign
  if ((rc = launch_infeas_roll(m, y_d.p, inf.yprev.p, aux.b_dev(*this), inf.dy.p, 0, 0, nullptr, nullptr, inf.partials.p, inf.stats_d.p + INF_DY2, st))) return rc;
  if ((rc = launch_infeas_roll(L, X.p, inf.xprev.p, C.p, dbuf, 1, 0, nullptr, nullptr, inf.partials.p, inf.stats_d.p + INF_DX2, st))) return rc;
  inf.checks++;
  double* hs = inf.h_stats.p;
  CUADMM_HIP_TRY(hipMemcpyAsync(hs, inf.stats_d.p, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  // a test's SpMV and projection run only when its scalar has the sign a certificate needs
  const bool try_dual = hs[INF_CDX] < 0 && hs[INF_DX2] > 0, try_primal = hs[INF_BDY] > 0 && hs[INF_DY2] > 0;
  int verdict = 0;
  double o3[3] = {0, 0, 0}, stats[INF_NSTATS];
  const double nan = std::nan("");
  // The dual test first: its input -dX sits in dbuf, which the primal test overwrites.
  if (try_dual) {      // A (-dX) over the whole svec; P+(-dX) with the unconstrained blocks' slices (copied through by the plan) left out
    if ((rc = launch_spmv_rows(m, A_avg_nnz, A_rp.p, A_ci.p, A_v.p, dbuf, S.p, C.p, inf.adx.p, nullptr, st, &A_long))) return rc;
    if ((rc = launch_infeas_norm2(m, inf.adx.p, inf.partials.p, inf.stats_d.p + INF_ADX2, st))) return rc;
    if ((rc = aux.project(*this, dbuf, pbuf))) return rc;
    for (auto& r : inf.free_rng) CUADMM_HIP_TRY(hipMemsetAsync(pbuf + r.first, 0, sizeof(double) * (size_t)r.second, st));
    if ((rc = launch_infeas_norm2(L, pbuf, inf.partials.p, inf.stats_d.p + INF_PNEGDX2, st))) return rc;
    CUADMM_HIP_TRY(hipMemcpyAsync(hs + INF_ADX2, inf.stats_d.p + INF_ADX2, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
    CUADMM_HIP_TRY(hipStreamSynchronize(st));
    for (int q = 0; q < INF_NSTATS; ++q) stats[q] = hs[q];
    stats[INF_DY2] = stats[INF_BDY] = stats[INF_PATY2] = nan; stats[INF_ATY2] = 0;
    if ((rc = infeas_decide(stats, inf.tol, &verdict, o3))) return rc;
  }
  if (verdict == 0 && try_primal) {   // A^T dy (the kernel forms A^T y - C: pbuf, zeroed, stands in for C), its PSD part, its norm
    CUADMM_HIP_TRY(hipMemsetAsync(pbuf, 0, sizeof(double) * (size_t)L, st));
    if ((rc = launch_aty_xb(false, L, At_rp.p, At_ci.p, At_v.p, inf.dy.p, pbuf, X.p, 1.0, dbuf, nullptr, st, &At_long))) return rc;
    if ((rc = launch_infeas_norm2(L, dbuf, inf.partials.p, inf.stats_d.p + INF_ATY2, st))) return rc;      // ||A^T dy||^2: the radius' rounding term
    if ((rc = aux.project(*this, dbuf, pbuf))) return rc;
    if ((rc = launch_infeas_norm2(L, pbuf, inf.partials.p, inf.stats_d.p + INF_PATY2, st))) return rc;
    CUADMM_HIP_TRY(hipMemcpyAsync(hs + INF_PATY2, inf.stats_d.p + INF_PATY2, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
    CUADMM_HIP_TRY(hipStreamSynchronize(st));
    for (int q = 0; q < INF_NSTATS; ++q) stats[q] = hs[q];
    stats[INF_DX2] = stats[INF_CDX] = stats[INF_ADX2] = stats[INF_PNEGDX2] = nan;
    if ((rc = infeas_decide(stats, inf.tol, &verdict, o3))) return rc;
  }
  float ms = 0;
  bool bad = false;
  if ((rc = aux.end(st, &ms, &bad))) return rc;
  inf.ms += ms;
  if (bad) { set_error("solve: a block projection of the infeasibility check hit the QL sweep cap"); return CUADMM_ERR_EIG; }
  if (verdict == 0) return CUADMM_OK;
  // the ray, as the check left it on the device (scaled space, the factor's order / the svec): dy, or -dX in dbuf
  const size_t n = verdict == 3 ? (size_t)m : (size_t)L;
  inf.cert.assign(n, 0.0);
  if ((rc = staged_d2h(inf.cert.data(), verdict == 3 ? inf.dy.p : dbuf, sizeof(double) * n, st))) return rc;
  if (verdict == 4) for (double& v : inf.cert) v = -v;
  solve_status = verdict; solve_status_iter = iter;
  inf.scalar = o3[0]; inf.eta = o3[1];
  // The reported radius is scalar / (eta + eta_fl): eta is the norm of a projection the kernels evaluate to 1e-12 ||M||_F per entry
  // (M = A^T dy or -dX: the projection's contract), so the true violation may exceed eta by eta_fl = 1e-12 sqrt(L) ||M||_F / ||d||, and
  // only the smaller radius is certified.  In the caller's units: X = bscale X_scaled (primal test); S = Cscale S_scaled,
  // y = Cscale y_scaled / normA (dual test).
  const double eta_fl = kInfeasProjErr * std::sqrt((double)L) * (verdict == 3 ? std::sqrt(stats[INF_ATY2] / stats[INF_DY2]) : 1.0);
  inf.radius = o3[0] / (o3[1] + eta_fl) * (verdict == 3 ? bscale : Cscale);
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// Certified lower bound from trace bounds (cuadmm_lower_bound, option "gap_check"): DESIGN.md, "Certified lower bound"
// ------------------------------------------------------------------------------------------
// vectors and task lists on first use; R and (the auxiliary projector's, where the engine keeps none on the device) b on every call: both may have changed
int cuadmm_solver::lb_prepare() {
  int rc;
  const int nb = (int)blk_local.size();
  if ((int)lb.R.size() != nb) { set_error("lower bound: %d trace bounds are set, the solver has %d blocks", (int)lb.R.size(), nb); return CUADMM_ERR_INVALID; }
  if (!lb.out_d.p) {
    const size_t mm = (size_t)std::max(m, 1);
    if (!btasks.built && (rc = btasks.build(blk_local.data(), nb, nullptr))) return rc;
    if ((rc = lb.ybuf.alloc(mm)) || (rc = lb.R_d.alloc((size_t)nb)) || (rc = lb.pairs.alloc(2 * (size_t)nb)) || (rc = lb.dpart.alloc(kBrSlots)) ||
        (rc = lb.h_out.alloc(4)) || (rc = lb.cpart.alloc(2 * (size_t)btasks.nchunk)))
      return rc;
    CUADMM_HIP_TRY(hipMemsetAsync(lb.pairs.p, 0, sizeof(double) * lb.pairs.n, st));
    lb.R_dirty = true;
    if ((rc = lb.out_d.alloc(4))) return rc;          // last: marks the set as complete
  }
  if (lb.R_dirty && (rc = staged_h2d(lb.R_d.p, lb.R.data(), sizeof(double) * (size_t)nb, st))) return rc;
  lb.R_dirty = false;
  return aux.ensure(*this);
}

// The bound at y (device, the engine's scaled space and the factor's order).  Reads y, A, C and b; writes only the bound's own vectors.
// out6 = [LB, b'y, sum R_k nubar_k, worst block, its term] in the caller's units, [5] unused.
int cuadmm_solver::lb_eval(const double* y, double out6[6], float* ms) {
  int rc;
  double* const mbuf = aux.in.p;
  double* const pbuf = aux.out.p;
  bool bad = false;
  if ((rc = aux.begin(st))) return rc;
  // M = A'y - C (S^ = -Cscale M), P = P+(M) with the unconstrained slices copied through
  if ((rc = dual_slack(y, lb.dpart.p)) || (rc = aux.project(*this, mbuf, pbuf))) return rc;
  if ((rc = launch_lb_block_norms(mbuf, pbuf, btasks.view(), lb.cpart.p, lb.pairs.p, st))) return rc;
  if ((rc = launch_lb_combine((int)blk_local.size(), lb.pairs.p, lb.R_d.p, btasks.len.p, btasks.blk.p, lb.dpart.p, lb.out_d.p, st))) return rc;
  CUADMM_HIP_TRY(hipMemcpyAsync(lb.h_out.p, lb.out_d.p, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
  if ((rc = aux.end(st, ms, &bad))) return rc;
  if (bad) { set_error("lower bound: a block projection hit the QL sweep cap"); return CUADMM_ERR_EIG; }
  const double* h = lb.h_out.p;
  out6[1] = h[3] * objscale;
  out6[2] = h[0] * Cscale;
  out6[0] = out6[1] - out6[2];
  out6[3] = h[1];
  out6[4] = h[2] * Cscale;
  out6[5] = 0;
  return CUADMM_OK;
}

// cuadmm_lower_bound's numbers at the scaled y in lb.ybuf; per_block: [nu_k, ||S^_k||_F] in the caller's units
int cuadmm_solver::lb_report(double o[8], double* per_block) {
  int rc;
  double r[6];
  float ms = 0;
  if ((rc = lb_eval(lb.ybuf.p, r, &ms))) return rc;
  o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
  o[3] = std::fabs(pobj - r[0]) / (1 + std::fabs(pobj) + std::fabs(r[0]));
  o[4] = r[3]; o[5] = r[4]; o[6] = ms; o[7] = lb.bytes() + btasks.bytes() + aux.bytes();
  if (per_block) {
    const size_t nb = blk_local.size();
    std::vector<double> pr(2 * nb);
    if ((rc = staged_d2h(pr.data(), lb.pairs.p, sizeof(double) * 2 * nb, st))) return rc;
    for (size_t k = 0; k < nb; ++k) { per_block[2 * k] = std::sqrt(pr[2 * k + 1]) * Cscale; per_block[2 * k + 1] = std::sqrt(pr[2 * k]) * Cscale; }
  }
  return CUADMM_OK;
}

// End of iteration `iter`, a multiple of the period: y_d holds this iteration's y (infeas_step), pobj and errRp are this iteration's.
int cuadmm_solver::lb_step(int iter, double stop_tol) {
  int rc;
  double o[6];
  float ms = 0;
  if ((rc = lb_eval(y_d.p, o, &ms))) return rc;
  lb.checks++;
  lb.ms += ms;
  const double LB = o[0], g = std::fabs(pobj - LB) / (1 + std::fabs(pobj) + std::fabs(LB));
  lb.last_lb = LB; lb.last_g = g;
  if (std::isfinite(LB) && (lb.best_iter == 0 || LB > lb.best_lb)) { lb.best_lb = LB; lb.best_iter = iter; }
  const double tol = lb.tol > 0 ? lb.tol : stop_tol;
  if (g <= tol && errRp <= tol) {          // (false for a NaN)
    solve_status = 5; solve_status_iter = iter;
    lb.verdict_iter = iter;
  }
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// Evaluation of a point (cuadmm_evaluate): DESIGN.md, "Evaluation of a point"
// ------------------------------------------------------------------------------------------
// vectors and task lists on first use; the column norms (where the engine keeps none on the device) and the auxiliary projector's b on
// every call: cuadmm_update_A / cuadmm_update_bC may have changed them
int cuadmm_solver::ev_prepare() {
  int rc;
  const int nb = (int)blk_local.size();
  const size_t mm = (size_t)std::max(m, 1);
  if (!ev.out_d.p) {
    if (!btasks.built && (rc = btasks.build(blk_local.data(), nb, nullptr))) return rc;
    if ((rc = ev.px.alloc((size_t)L)) || (rc = ev.cons.alloc(mm)) || (!normA_d.p && (rc = ev.normA.alloc(mm))) || (rc = ev.sums.alloc(kEvSums * (size_t)nb)) ||
        (rc = ev.cpart.alloc(kEvSums * (size_t)btasks.nchunk)) || (rc = ev.part.alloc(3 * (size_t)kBrSlots)) || (rc = ev.h_out.alloc(kEvGlobals)))
      return rc;
    CUADMM_HIP_TRY(hipMemsetAsync(ev.sums.p, 0, sizeof(double) * ev.sums.n, st));      // (a block without slots keeps zeros)
    if ((rc = ev.out_d.alloc(kEvGlobals))) return rc;      // last: marks the set as complete
  }
  if (ev.normA.p && m > 0 && (rc = staged_h2d(ev.normA.p, normA_p.data(), sizeof(double) * (size_t)m, st))) return rc;
  return aux.ensure(*this);
}

// One svec vector of the point in the engine's scaled space.  host: the caller's (this rank's L entries), scaled as init scales X0 / S0,
// into `own`; null: the resident one -- read where it lies when a solve left it scaled, else a scaled copy in `own`.
int cuadmm_solver::ev_point(const double* host, const DevBuf<double>& resident, double inv_scale, DevBuf<double>& own, const double** out) {
  int rc;
  if (!host && pending_unscale) { *out = resident.p; return CUADMM_OK; }
  if (!own.p && (rc = own.alloc((size_t)L))) return rc;
  if (host) {
    std::vector<double> tmp((size_t)L);
    for (long long i = 0; i < L; ++i) tmp[i] = host[i] * inv_scale;
    if ((rc = staged_h2d(own.p, tmp.data(), sizeof(double) * (size_t)L, st))) return rc;
  } else {
    CUADMM_HIP_TRY(hipMemcpyAsync(own.p, resident.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, st));
    if ((rc = launch_scale(own.p, L, inv_scale, st))) return rc;
  }
  *out = own.p;
  return CUADMM_OK;
}

// The report at (xs, y in ev.cons, ss), all scaled and in the engine's order.  Reads A, A', b, C; writes only the evaluation's and the
// auxiliary projector's vectors.  The scalars go back to the caller's units as set_residual_scalars and lb_eval convert theirs:
// X = bscale X_s, S = Cscale S_s, Rd = Cscale Rd_s, objectives and <X, S> times objscale; ev_rp forms ||A X - b|| in them itself.
int cuadmm_solver::ev_run(const double* xs, const double* ss, double o[16], double* per_block) {
  int rc;
  const int nb = (int)blk_local.size();
  double* const cons = ev.cons.p;
  double* const rd1 = aux.in.p;      // A'y - C
  double* const ps = aux.out.p;      // P+(S)
  double *const cx_part = ev.part.p, *const by_part = ev.part.p + kBrSlots, *const rp_part = ev.part.p + 2 * kBrSlots;
  const double* const normA_dev = normA_d.p ? normA_d.p : ev.normA.p;
  float ms = 0;
  bool bad = false;
  if ((rc = aux.begin(st)) || (rc = dual_slack(cons, by_part))) return rc;
  if ((rc = launch_lb_dot(L, C.p, xs, cx_part, st))) return rc;
  // A X from the engine's whole A (kept in every mode: the fused and closed iterations evaluate rows of it elsewhere), over y in cons
  if (m > 0 && (rc = launch_spmv_rows(m, A_avg_nnz, A_rp.p, A_ci.p, A_v.p, xs, ss, C.p, cons, nullptr, st, &A_long))) return rc;
  if ((rc = launch_ev_rp(m, cons, aux.b_dev(*this), normA_dev, bscale, rp_part, st))) return rc;
  if ((rc = aux.project(*this, xs, ev.px.p))) return rc;
  if ((rc = aux.project(*this, ss, ps))) return rc;
  if ((rc = launch_ev_block_stats(xs, ss, ev.px.p, ps, rd1, btasks.view(), ev.cpart.p, ev.sums.p, st))) return rc;
  if ((rc = launch_ev_combine(nb, ev.sums.p, cx_part, by_part, rp_part, ev.out_d.p, st))) return rc;
  CUADMM_HIP_TRY(hipMemcpyAsync(ev.h_out.p, ev.out_d.p, sizeof(double) * kEvGlobals, hipMemcpyDeviceToHost, st));
  if ((rc = aux.end(st, &ms, &bad))) return rc;
  ev.ms = ms;
  ev.calls++;
  if (bad) { set_error("evaluate: a block projection hit the QL sweep cap"); return CUADMM_ERR_EIG; }
  const double* h = ev.h_out.p;
  const double nb1 = norm_borg, nc1 = norm_Corg;      // 1 + ||b||, 1 + ||C||
  o[0] = h[4] * objscale;
  o[1] = h[5] * objscale;
  o[2] = std::sqrt(h[6]);
  o[3] = std::sqrt(h[3]) * Cscale;
  o[4] = std::sqrt(h[0]) * bscale;
  o[5] = std::sqrt(h[1]) * Cscale;
  o[6] = h[2] * objscale;
  o[7] = nb1 - 1;
  o[8] = nc1 - 1;
  const double den = 1 + std::fabs(o[0]) + std::fabs(o[1]);
  o[9] = o[2] / nb1; o[10] = o[4] / nb1; o[11] = o[3] / nc1; o[12] = o[5] / nc1;
  o[13] = (o[0] - o[1]) / den; o[14] = o[6] / den;
  o[15] = ev.ms;
  if (per_block) {
    std::vector<double> q(kEvSums * (size_t)nb);
    if (nb > 0 && (rc = staged_d2h(q.data(), ev.sums.p, sizeof(double) * q.size(), st))) return rc;
    for (size_t k = 0; k < (size_t)nb; ++k) {
      const double* v = q.data() + kEvSums * k;
      double* w = per_block + kEvSums * k;
      w[0] = std::sqrt(v[0]) * bscale; w[1] = std::sqrt(v[1]) * bscale; w[2] = std::sqrt(v[2]) * Cscale; w[3] = std::sqrt(v[3]) * Cscale;
      w[4] = v[4] * objscale; w[5] = std::sqrt(v[5]) * Cscale;
    }
  }
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// Certified lambda_min per block (cuadmm_lambda_min): DESIGN.md, "Certified lambda_min"
// ------------------------------------------------------------------------------------------
// lists and vectors on first use; the auxiliary projector's events, vectors and b (which may have changed) on every call
int cuadmm_solver::lm_prepare(int which) {
  int rc;
  const int nb = (int)blk_local.size();
  if (!btasks.built && (rc = btasks.build(blk_local.data(), nb, nullptr))) return rc;
  if (!lm.out.p && (rc = lm.build(blk_local.data(), nb))) return rc;
  if (which == 2 && !lm.dpart.p && ((rc = lm.ybuf.alloc((size_t)std::max(m, 1))) || (rc = lm.dpart.alloc(kBrSlots)))) return rc;
  return aux.ensure(*this);
}

// which = 0: X, 1: S, read where they lie (scaled behind a solve, else in the caller's units); 2: S^ = C - A'y at the scaled y in lm.ybuf,
// formed as -(A'y - C) by the iteration's kernel into the auxiliary projector's input vector.  The kernel's numbers are in the units of
// the vector it read; lo goes to the caller's units rounded down.  Writes only the plan's own vectors and that input vector.
int cuadmm_solver::lm_run(int which, int steps, double o[8], double* per_block) {
  int rc;
  const int nb = (int)blk_local.size();
  const double* v = which == 0 ? X.p : S.p;
  double sign = 1.0, unit = pending_unscale ? (which == 0 ? bscale : Cscale) : 1.0;
  float ms = 0;
  if ((rc = aux.begin(st))) return rc;
  if (which == 2) {
    if ((rc = dual_slack(lm.ybuf.p, lm.dpart.p))) return rc;
    v = aux.in.p; sign = -1.0; unit = Cscale;
  }
  if ((rc = lm.run(v, sign, btasks.off.p, btasks.blk.p, steps, st))) return rc;
  double* const h = lm.h_out.p;
  CUADMM_HIP_TRY(hipMemcpyAsync(h, lm.out.p, sizeof(double) * kLmOut * (size_t)nb, hipMemcpyDeviceToHost, st));
  if (which == 2) CUADMM_HIP_TRY(hipMemcpyAsync(h + kLmOut * (size_t)nb, lm.dpart.p, sizeof(double) * kBrSlots, hipMemcpyDeviceToHost, st));
  if ((rc = aux.end(st, &ms, nullptr))) return rc;
  lm.calls++;
  const bool bound = which == 2 && !lb.R.empty();
  double worst = INFINITY, pen = 0;
  int arg = -1, unrefined = 0, at_floor = 0;
  for (int k = 0; k < nb; ++k) {
    const double* q = h + kLmOut * (size_t)k;
    const int flag = (int)q[2];
    double lo = q[0] * unit, hi = q[1] * unit;
    if (unit != 1.0 && flag != kLmFree) lo = std::nextafter(lo, -INFINITY);
    if (flag != kLmFree && lo < worst) { worst = lo; arg = k; }
    unrefined += flag == kLmUnrefined; at_floor += flag == kLmPsdAtFloor;
    if (bound) pen += lb.R[k] * (flag == kLmFree ? q[3] * unit : std::max(0.0, -lo));
    if (per_block) { per_block[3 * k] = lo; per_block[3 * k + 1] = hi; per_block[3 * k + 2] = (double)flag; }
  }
  o[0] = arg >= 0 ? worst : 0.0;
  o[1] = (double)arg;
  o[2] = std::max(0.0, -o[0]) / (which == 0 ? norm_borg : norm_Corg);
  o[3] = NAN;
  if (bound) {
    double by = 0;
    for (int j = 0; j < kBrSlots; ++j) by += h[kLmOut * (size_t)nb + j];
    o[3] = by * objscale - pen;
  }
  o[4] = (double)unrefined; o[5] = (double)at_floor;
  o[6] = ms;
  o[7] = lm.bytes() + btasks.bytes() + aux.bytes();
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// Rank and low-rank factor per block (cuadmm_lowrank): DESIGN.md, "Low-rank factors"
// ------------------------------------------------------------------------------------------
// lists, events and buffers on first use; offsets and larger buffers when rmax changes
int cuadmm_solver::lr_prepare(int rmax) {
  int rc;
  const int nb = (int)blk_local.size();
  if (!btasks.built && (rc = btasks.build(blk_local.data(), nb, nullptr))) return rc;
  return lr.prepare(blk_local.data(), nb, rmax);
}

// which = 0: X, 1: S, read where they lie (scaled behind a solve, else in the caller's units).  The kernel's numbers are in the units of the
// vector it read: M = unit M_s, so L = sqrt(unit) L_s and the residual diagonal, its sums and the trace take the factor unit.  Writes only
// the plan's own buffers.
int cuadmm_solver::lr_run(int which, double tol, double o[8], double* per_block, double* L_out, int* piv_out) {
  int rc;
  const int nb = (int)blk_local.size();
  const double* v = which == 0 ? X.p : S.p;
  const double unit = pending_unscale ? (which == 0 ? bscale : Cscale) : 1.0;
  CUADMM_HIP_TRY(hipEventRecord(lr.ev[0], st));
  if ((rc = lr.run(v, 1.0, btasks.off.p, btasks.blk.p, tol, st))) return rc;
  CUADMM_HIP_TRY(hipEventRecord(lr.ev[1], st));
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  const float ms = event_ms(lr.ev[0], lr.ev[1]);
  lr.calls++;
  std::vector<double> own;
  if (!per_block) { own.resize(kLrOut * (size_t)nb); per_block = own.data(); }
  if ((rc = lr.fetch(unit, per_block, L_out, piv_out))) return rc;
  double sum_r = 0, max_r = 0, resid = 0, dneg = 0;
  int arg = -1, capped = 0;
  for (int k = 0; k < nb; ++k) {
    const double* q = per_block + kLrOut * (size_t)k;
    if ((int)q[4] == kLrFree) continue;
    sum_r += q[0];
    if (arg < 0 || q[0] > max_r) { max_r = q[0]; arg = k; }
    resid += q[1];
    if (q[2] < dneg) dneg = q[2];
    capped += (int)q[4] == kLrCapped;
  }
  o[0] = sum_r; o[1] = max_r; o[2] = (double)arg; o[3] = resid; o[4] = dneg; o[5] = (double)capped;
  o[6] = ms;
  o[7] = lr.bytes() + btasks.bytes();
  return CUADMM_OK;
}

// SDPDuoSolver front (duo_solver.h:236-276): exactly two block sizes, then the generic engine.
int cuadmm_duo_init(cuadmm_solver* s, int if_gpu_eig_mom, int device_num_requested, int eig_stream_num_per_gpu,
                    int cpu_eig_thread_num, int vec_len, int con_num, const int* At_cp, const int* At_ri, const double* At_vx,
                    int At_nnz, const int* b_idx, const double* b_vals, int b_nnz, const int* C_idx, const double* C_vals,
                    int C_nnz, const int* blk, int mat_num, const double* X0, const double* y0, const double* S0, double sig) {
  if (!s || !blk || mat_num <= 0) { set_error("duo_init: invalid argument"); return CUADMM_ERR_INVALID; }
  // if_gpu_eig_mom = false asks for the reference's host-LAPACK moment-matrix path (duo_solver.cu:578-618,793-834).  This engine
  // has no CPU projection (and no CPU fallback by design): say so instead of silently running the GPU kernels; the option
  // "duo_cpu_eig_on_gpu" = 1 accepts the request and projects on the GPU (same iterates, to the projection's tolerance).
  if (!if_gpu_eig_mom && !s->duo_cpu_eig_on_gpu) {
    set_error("duo_init: if_gpu_eig_mom = false selects the reference's host LAPACK eigendecomposition; this engine projects on the GPU only "
              "(set option duo_cpu_eig_on_gpu = 1 to run the GPU projection for such a call)");
    return CUADMM_ERR_INVALID;
  }
  // duo_solver.cu:487-577 spreads the moment matrices over device_num_requested GPUs from ONE process (threads + P2P copies,
  // check_gpus.cu:29-43).  Here a GPU is a rank of the block-sharded engine: with rank / world already set by the caller (one
  // process per GPU) the request must agree with them; from a single process (world = 1) the handle becomes rank 0 of a GROUP of
  // N engines on N host threads with an in-process all-reduce (duo_group.hip).
  if (device_num_requested > 1 && s->aa.mem > 0) {
    set_error("duo_init: option accel works on one engine (device_num_requested = %d): its Gram matrix is not all-reduced", device_num_requested);
    return CUADMM_ERR_INVALID;
  }
  if (device_num_requested > 1 && s->inf.period > 0) {
    set_error("duo_init: option infeas_check works on one engine (device_num_requested = %d): its sums are not all-reduced", device_num_requested);
    return CUADMM_ERR_INVALID;
  }
  if (device_num_requested > 1 && s->lb.period > 0) {
    set_error("duo_init: option gap_check works on one engine (device_num_requested = %d): its sums are not all-reduced", device_num_requested);
    return CUADMM_ERR_INVALID;
  }
  if (device_num_requested > 1 && s->world == 1 && !s->in_group_call) {
    if (s->group) { set_error("duo_init: this handle already leads a group of %d engines", duo_group_world(s->group)); return CUADMM_ERR_INVALID; }
    if (s->initialised) { set_error("duo_init: already initialised"); return CUADMM_ERR_INVALID; }
    DeviceGuard keep_device;                // the ranks' devices are made current on this thread: leave the caller's as it was
    int rc = duo_group_create(s, device_num_requested, s->device, s->duo_share_device != 0, s->duo_exchange, s->option_log, &s->group);
    if (rc) return rc;
    duo_group_inject(s->group, s->duo_inject);
    s->world = device_num_requested; s->rank = 0;
    rc = group_forward(s, [&](cuadmm_solver* q) {
      return cuadmm_duo_init(q, if_gpu_eig_mom, device_num_requested, eig_stream_num_per_gpu, cpu_eig_thread_num, vec_len, con_num, At_cp, At_ri,
                             At_vx, At_nnz, b_idx, b_vals, b_nnz, C_idx, C_vals, C_nnz, blk, mat_num, X0, y0, S0, sig);
    });
    if (rc) { duo_group_destroy(s->group); s->group = nullptr; s->world = 1; s->allreduce = nullptr; s->allreduce_user = nullptr; }
    return rc;
  }
  if (device_num_requested > 1 && device_num_requested != s->world) {
    set_error("duo_init: device_num_requested = %d but this handle is rank %d of %d: one process per GPU needs world = device_num_requested "
              "(or leave world = 1 and let duo_init build the in-process group)", device_num_requested, s->rank, s->world);
    return CUADMM_ERR_INVALID;
  }
  std::vector<int> sizes, nums;
  analyze_blk(blk, mat_num, sizes, nums);
  if (sizes.size() != 2) {   // analyze_blk_duo, src/utils/analyze_blk.cu:39-43
    set_error("SDP solver only supports two matrix sizes! You matrix type number is: %d", (int)sizes.size());
    return CUADMM_ERR_INVALID;
  }
  if (s->verbose && s->rank == 0) {
    std::cout << "\nAnalysis of the blk vector:" << std::endl;
    std::cout << "moment matrix size: " << sizes[1] << std::endl;
    std::cout << "localizing matrix size: " << sizes[0] << std::endl;
    std::cout << "number of moment matrices: " << nums[1] << std::endl;
    std::cout << "number of localizing matrices: " << nums[0] << std::endl << std::endl;
  }
  const int verbose = s->verbose;
  s->verbose = 0;   // the generic census is not part of the duo solver's console output
  int rc = cuadmm_init(s, eig_stream_num_per_gpu, cpu_eig_thread_num, vec_len, con_num, At_cp, At_ri, At_vx, At_nnz, b_idx, b_vals,
                       b_nnz, C_idx, C_vals, C_nnz, blk, mat_num, X0, y0, S0, sig);
  s->verbose = verbose;
  return rc;
}
int cuadmm_duo_solve(cuadmm_solver* s, int max_iter, double stop_tol, int sig_update_threshold, int sig_update_stage_1,
                     int sig_update_stage_2, int switch_admm, double sigscale, int if_first) {
  return cuadmm_solve(s, max_iter, stop_tol, sig_update_threshold, sig_update_stage_1, sig_update_stage_2, switch_admm, sigscale, if_first);
}

int cuadmm_get_dims(const cuadmm_solver* s, int* vec_len, int* con_num, int* mat_num) {
  if (!s) { set_error("get_dims: null"); return CUADMM_ERR_INVALID; }
  // the caller's numbering in every sharding mode: cuadmm_get_y writes con_num doubles, cuadmm_set_XyS / cuadmm_get_shard
  // index the global svec
  if (vec_len) *vec_len = s->local_mode ? s->L_caller : s->L_full;
  if (con_num) *con_num = s->local_mode ? s->m_full : s->m;
  if (mat_num) *mat_num = s->local_mode ? s->nblk_caller : s->nblk_full;
  return CUADMM_OK;
}

static int get_vec(cuadmm_solver* s, const DevBuf<double>& v, double* out) {
  if (!s || !s->initialised || !out) { set_error("get: bad arguments"); return CUADMM_ERR_INVALID; }
  int rc = check_device(s->device);
  if (rc) return rc;
  if ((rc = s->materialise())) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(s->st));
  if (s->L > 0) { int rc2 = staged_d2h(out, v.p, sizeof(double) * (size_t)s->L, s->st); if (rc2) return rc2; }
  return CUADMM_OK;
}
// world>1: writes this rank's shard (length svec_end - svec_begin) at out[0..)
// the leader of an in-process group gathers the shards: out has the caller's vec_len doubles
static int group_gather(cuadmm_solver* s, double* out, int (*get)(cuadmm_solver*, double*)) {
  DeviceGuard keep_device;                  // every rank's getter makes its device current on this thread
  for (int r = 0; r < duo_group_world(s->group); ++r) {
    // (rank 0 IS the leader: without the mark get_shard would answer for the whole group)
    int rc = as_group_rank(duo_group_rank(s->group, r), [&](cuadmm_solver* q) {
      int64_t b = 0, e = 0;
      const int rs = cuadmm_get_shard(q, &b, &e, nullptr, nullptr);
      return rs ? rs : (e > b ? get(q, out + b) : CUADMM_OK);
    });
    if (rc) return rc;
  }
  return CUADMM_OK;
}
int cuadmm_get_X(cuadmm_solver* s, double* out) {
  if (s && s->group && !s->in_group_call) return group_gather(s, out, cuadmm_get_X);
  return get_vec(s, s->X, out);
}
int cuadmm_get_S(cuadmm_solver* s, double* out) {
  if (s && s->group && !s->in_group_call) return group_gather(s, out, cuadmm_get_S);
  return get_vec(s, s->S, out);
}
int cuadmm_get_y(cuadmm_solver* s, double* out) {
  if (!s || !s->initialised || !out) { set_error("get_y: bad arguments"); return CUADMM_ERR_INVALID; }
  { int rc = s->materialise(); if (rc) return rc; }
  if (s->local_mode) {
    if ((int)s->y_full.size() == s->m_full) std::copy(s->y_full.begin(), s->y_full.end(), out);   // gathered at the end of solve
    else { std::fill(out, out + s->m_full, 0.0); for (int i = 0; i < s->m; ++i) out[s->cons_local[s->perm[i]]] = s->y_p[i]; }
    return CUADMM_OK;
  }
  for (int i = 0; i < s->m; ++i) out[s->perm[i]] = s->y_p[i];          // y[perm[i]] = y_perm[i], solver.cu:500
  return CUADMM_OK;
}

int cuadmm_set_XyS(cuadmm_solver* s, const double* X, const double* y, const double* S, double sig) {
  if (!s || !s->initialised) { set_error("set_XyS: not initialised"); return CUADMM_ERR_INVALID; }
  if (s->group && !s->in_group_call) {      // every rank of the group takes its range of the caller's vectors
    DeviceGuard keep_device;
    for (int r = 0; r < duo_group_world(s->group); ++r) {
      int rc = as_group_rank(duo_group_rank(s->group, r), [&](cuadmm_solver* q) { return cuadmm_set_XyS(q, X, y, S, sig); });
      if (rc) return rc;
    }
    return CUADMM_OK;
  }
  int rc = check_device(s->device);
  if (rc) return rc;
  if ((rc = s->materialise())) return rc;       // the vectors NOT replaced must be in the caller's units too
  if (X && s->L > 0) { int rc2 = staged_h2d(s->X.p, X + s->sv_off + s->sv_begin, sizeof(double) * (size_t)s->L, s->st); if (rc2) return rc2; }
  if (S && s->L > 0) { int rc2 = staged_h2d(s->S.p, S + s->sv_off + s->sv_begin, sizeof(double) * (size_t)s->L, s->st); if (rc2) return rc2; }
  if (y) for (int i = 0; i < s->m; ++i) s->y_p[i] = s->local_mode ? y[s->cons_local[s->perm[i]]] : y[s->perm[i]];
  if (sig > 0) s->sig = sig;
  s->infeas_reset();                            // snapshots and status describe another iterate
  s->lb_reset();
  return CUADMM_OK;
}

// New b and / or C on a factored solver.  Nothing that depends on A alone is touched: ordering, factor, GPU tail, tree tops, CSR
// matrices, projection plan.  What changes: the scaling constants, b (host, device, the closed blocks' records), C, the units of the
// resident X, y, S -- rescaled where they live, with the rounded operations of materialise() followed by init's scaling -- and the
// per-solve bookkeeping, which goes back to what init leaves.  The last stage of init (init_residuals) then runs as it does there.
int cuadmm_update_bC(cuadmm_solver* s, const int* b_idx, const double* b_vals, int b_nnz, const int* C_idx, const double* C_vals, int C_nnz,
                     int keep_iterate, double sig) {
  if (!s || !s->initialised) { set_error("update_bC: solver not initialised"); return CUADMM_ERR_INVALID; }
  if (s->factor_bad) { set_error("update_bC: the last cuadmm_update_A could not factor the new A A^T; the solver needs a successful cuadmm_update_A first"); return CUADMM_ERR_FACTOR; }
  const bool new_b = b_nnz >= 0, new_C = C_nnz >= 0;
  if ((b_nnz > 0 && (!b_idx || !b_vals)) || (C_nnz > 0 && (!C_idx || !C_vals))) { set_error("update_bC: entries without their index / value arrays"); return CUADMM_ERR_INVALID; }
  // --- every check before anything changes (the caller's numbering; the rules of init_vectors, over the whole of b and C on every rank)
  int rc;
  if (new_b && (rc = check_sparse_idx("update_bC", "b", b_idx, b_nnz, s->local_mode ? s->m_full : s->m))) return rc;
  if (new_C && (rc = check_sparse_idx("update_bC", "C", C_idx, C_nnz, s->local_mode ? s->L_caller : s->L_full))) return rc;
  if (s->group && !s->in_group_call)        // every rank takes the full b and C, as with init; their residual stage meets in the group's all-reduce
    return group_forward(s, [&](cuadmm_solver* q) { return cuadmm_update_bC(q, b_idx, b_vals, b_nnz, C_idx, C_vals, C_nnz, keep_iterate, sig); });
  if ((rc = check_device(s->device))) return rc;
  const double t_begin = wall_s();
  const int m = s->m;
  const long long L = s->L;

  // --- this rank's entries, in the engine's numbering: b by position in the factor's order and divided by normA, C by local svec slot; the
  // norms over the WHOLE of b and C (owned constraints: from the full inputs every rank holds)
  const int* const g2l = s->local_mode ? s->cons_g2l.data() : nullptr;
  double nb = 0, nb2 = 0, nc = 0;
  std::vector<int> bi, ci;
  std::vector<double> bv, cv, bfull;
  if (new_b) {
    nb = sum_sq(b_vals, b_nnz);
    nb2 = scaled_b(b_idx, b_vals, b_nnz, g2l, s->normA, bfull);
    if (s->local_mode) nb2 = sum_scaled_sq(b_idx, b_vals, b_nnz, s->normA_all.data());
    for (int i = 0; i < b_nnz; ++i) {
      const int j = g2l ? g2l[b_idx[i]] : b_idx[i];
      if (j >= 0) { bi.push_back(s->perm_inv[j]); bv.push_back(bfull[j]); }
    }
  }
  if (new_C) {
    const long long lo = s->sv_off + s->sv_begin, hi = s->sv_off + s->sv_end;
    for (int i = 0; i < C_nnz; ++i) {
      nc += C_vals[i] * C_vals[i];
      if (C_idx[i] >= lo && C_idx[i] < hi) { ci.push_back((int)(C_idx[i] - lo)); cv.push_back(C_vals[i]); }
    }
  }
  // the sparse entries are all that crosses to the device
  DevBuf<int> bi_d, ci_d;
  DevBuf<double> bv_d, cv_d;
  const bool b_on_device = new_b && s->b_d.p != nullptr;
  s->prof_begin(K_COPY);
  if (b_on_device && !bi.empty() && ((rc = bi_d.from(bi)) || (rc = bv_d.from(bv)))) return rc;
  if (!ci.empty() && ((rc = ci_d.from(ci)) || (rc = cv_d.from(cv)))) return rc;
  s->prof_end(K_COPY, 12.0 * ((b_on_device ? (double)bi.size() : 0.0) + (double)ci.size()));

  // --- from here on the solver changes.  A solve left X, y, S scaled (pending): their way back to the caller's units is folded into
  // the rescaling; otherwise they are taken as they stand, as init takes X0, y0, S0.
  const bool pending = s->pending_unscale;
  if (!pending && (rc = s->sync_y_host())) return rc;
  const double bs_old = s->bscale, cs_old = s->Cscale;
  if (new_b) {
    if (!s->local_mode) { s->upa.b_idx.assign(b_idx, b_idx + b_nnz); s->upa.b_val.assign(b_vals, b_vals + b_nnz); }   // what a later cuadmm_update_A rescales
    else {
      s->upa.bg_idx.assign(b_idx, b_idx + b_nnz); s->upa.bg_val.assign(b_vals, b_vals + b_nnz);
      s->upa.b_idx.clear(); s->upa.b_val.clear();
      for (int i = 0; i < b_nnz; ++i) if (g2l[b_idx[i]] >= 0) { s->upa.b_idx.push_back(g2l[b_idx[i]]); s->upa.b_val.push_back(b_vals[i]); }
    }
    s->norm_borg = 1 + std::sqrt(nb);
    s->set_scaled_b(bfull, nb2);
    if (s->local_mode) { s->ov_nb = nb; s->ov_nb2 = nb2; }
  }
  if (new_C) {
    s->norm_Corg = 1 + std::sqrt(nc);
    s->Cscale = 1 + std::sqrt(nc);
    if (s->local_mode) s->ov_nc = nc;
  }
  s->objscale = s->bscale * s->Cscale;
  const double ibs = 1 / s->bscale, ics = 1 / s->Cscale;

  // svec pass: X, S (and C <- 0), then C's entries
  const bool keep = keep_iterate != 0;
  s->prof_begin(K_POST);
  if ((rc = launch_update_svec(s->X.p, s->S.p, new_C ? s->C.p : nullptr, L, !keep, pending ? bs_old : 1.0, ibs, pending ? cs_old : 1.0, ics, s->st))) return rc;
  s->prof_end(K_POST, (new_C ? 40.0 : 32.0) * (double)L);
  if (new_C && (rc = launch_scatter_scaled(s->C.p, ci_d.p, cv_d.p, (int)ci.size(), ics, s->st))) return rc;

  // constraint pass: b_d and y where they live
  const bool y_on_device = s->dev_solve && (pending || !keep);
  if (y_on_device) {
    if ((rc = launch_update_cons(m, b_on_device ? s->b_d.p : nullptr, s->y_d.p, s->normA_d.p, keep ? 2 : 1, cs_old, ics, s->st))) return rc;
    if (!keep) std::fill(s->y_p.begin(), s->y_p.end(), 0.0);
    s->y_host_stale = keep && m > 0;
  } else {
    if (pending && !s->dev_solve)      // the solve left y_p scaled
      for (int i = 0; i < m; ++i) s->y_p[i] = s->y_p[i] / s->normA_p[i] * cs_old;
    if (keep) for (int i = 0; i < m; ++i) s->y_p[i] = (s->y_p[i] * s->normA_p[i]) * ics;
    else std::fill(s->y_p.begin(), s->y_p.end(), 0.0);
    if (b_on_device && (rc = launch_update_cons(m, s->b_d.p, nullptr, nullptr, 0, cs_old, ics, s->st))) return rc;
  }
  if (b_on_device) {
    if ((rc = launch_scatter_scaled(s->b_d.p, bi_d.p, bv_d.p, (int)bi.size(), ibs, s->st))) return rc;
    if (s->closed.active && (rc = launch_closed_patch_b(s->closed.rec.p, s->plan.fused_blocks(), s->b_d.p, s->st))) return rc;
  }
  s->pending_unscale = false;           // (y_host_stale: set above, by where y lives)
  if (sig > 0) s->sig = sig;
  if ((rc = s->reset_solve_state(t_begin))) return rc;

  // --- initial A X, A (S - C), residual scalars: init's own last stage (it ends with a stream synchronisation)
  return init_residuals(s, y_on_device);
}


// New values of A on the pattern of init.  Everything that depends on the pattern alone stays: the pattern of A A^T, the ordering, the
// elimination tree and column counts, the tail cut and the tops plan, the projection plan, the closed-block and fused-row
// classification, the index arrays of both device matrices.  What is formed again, by the routines of init in their arithmetic order:
// the column norms and the normalised values, the host factor (cuadmm_aat_refactor), the GPU tail with its probe solve, the streams of the
// device-side y-solve, the value arrays of A and A^T (one upload of the normalised values, one kernel through two index maps), the
// closed blocks' records, b and the scaling constants, the units of X, y, S.  Decisions of init that depend on VALUES are taken again
// (DESIGN.md section 7 lists them); where one comes out differently the handle would need another plan, which only an init builds:
// the call then fails like a factorisation that broke down and the solver refuses to solve until an update succeeds.
int cuadmm_update_A(cuadmm_solver* s, const double* At_vals, int At_nnz, int keep_iterate, double sig) {
  if (!s || !s->initialised) { set_error("update_A: solver not initialised"); return CUADMM_ERR_INVALID; }
  // --- every check before anything changes
  const int nnz_init = s->local_mode ? s->upa.g_cp.back() : (int)s->upa.ri.size();
  if (At_nnz != nnz_init) { set_error("update_A: %d values, the pattern given to init has %d entries", At_nnz, nnz_init); return CUADMM_ERR_INVALID; }
  if (At_nnz > 0 && !At_vals) { set_error("update_A: null values"); return CUADMM_ERR_INVALID; }
  for (int p = 0; p < At_nnz; ++p)
    if (!std::isfinite(At_vals[p])) { set_error("update_A: value %d is not finite", p); return CUADMM_ERR_INVALID; }
  // (init keeps explicit zeros in the pattern -- of A, of A A^T and of the factor --, so a value of exactly 0 is as good as any other)
  if (s->group && !s->in_group_call)        // every rank takes the full value array, as with init
    return group_forward(s, [&](cuadmm_solver* q) { return cuadmm_update_A(q, At_vals, At_nnz, keep_iterate, sig); });
  if (s->upa.tail_fellback) {
    set_error("update_A: init fell back from the GPU tail to the host-only factor on the values it was given; whether new values would take the tail is a decision only an init can take");
    return CUADMM_ERR_INVALID;
  }
  int rc = check_device(s->device);
  if (rc) return rc;
  const double t_begin = wall_s();
  const int m = s->m;
  const long long L = s->L;
  const bool keep = keep_iterate != 0;
  s->upa.bytes = 0;

  // X, y, S to the caller's units where a solve left them scaled (the rounded operations a caller reading them would have seen)
  if ((rc = s->materialise())) return rc;

  // owned constraints: the norms of EVERY constraint and the sum behind bscale from the full inputs, then this rank's own values
  std::vector<double> local_vals;
  if (s->local_mode) {
    const int* gcp = s->upa.g_cp.data();
    for (int j = 0; j < s->m_full; ++j) s->normA_all[j] = cons_norm(At_vals, gcp[j], gcp[j + 1]);
    s->ov_nb2 = sum_scaled_sq(s->upa.bg_idx.data(), s->upa.bg_val.data(), (int)s->upa.bg_idx.size(), s->normA_all.data());
    local_vals.resize(s->upa.g_from.size());
    for (size_t p = 0; p < local_vals.size(); ++p) local_vals[p] = At_vals[s->upa.g_from[p]];
    At_vals = local_vals.data();
    At_nnz = (int)local_vals.size();
  }
  // --- column norms, normalised values, A^T by svec rows: init's own stage
  s->upa.in_update = true;
  struct Leave { cuadmm_solver* s; int verbose; ~Leave() { s->upa.in_update = false; s->verbose = verbose; } } leave{s, s->verbose};
  s->verbose = 0;                                              // the stages of init print their plans; they are not new
  InitIn in{s->L_full, m, At_nnz, (int)s->upa.b_idx.size(), 0, (int)s->blk_local.size(), s->upa.cp.data(), s->upa.ri.data(), s->upa.b_idx.data(), nullptr,
            s->blk_local.data(), At_vals, s->upa.b_val.data(), nullptr, nullptr, nullptr, nullptr, s->sig};
  InitCtx ctx;
  const std::vector<double> normA_old = s->normA;
  if ((rc = init_normalise(s, in, ctx))) return rc;

  // --- host factor on the analysis of init, then the GPU tail from the new Schur complement through init's routine and probe
  s->factor_bad = true;                                        // until every stage below has gone through
  auto fail = [&](int code) { s->normA = normA_old; return code; };
  const double t_f0 = wall_s();
  double t_f1 = t_f0;
  auto factor_stage = [&]() -> int {
    int rc = CUADMM_OK;
    if ((rc = cuadmm_aat_refactor(s->fac, ctx.rv.data()))) return (rc);
    t_f1 = wall_s();
    const int inject = s->upa.inject_fail;
    s->upa.inject_fail = 0;
    if (inject == 1) { set_error("update_A: injected failure behind the host refactorisation (test hook)"); return CUADMM_ERR_FACTOR; }
    if (s->tail.k > 0) {
      const int tk = cuadmm_aat_tail_k(s->fac);
      const int64_t* srp; const int* sci; const double* sv;
      if ((rc = cuadmm_aat_tail_schur(s->fac, &srp, &sci, &sv))) return (rc);
      s->tail.shard_rank = 0; s->tail.shard_world = 1; s->tail.reduce_fn = nullptr;      // as at init: the probe applies the whole tail; solve sets the shard again
      rc = s->tail.build_from_schur(reinterpret_cast<const long long*>(srp), sci, sv, tk, s->st);
      bool tail_ok = rc == CUADMM_OK;
      if (rc == CUADMM_OK) rc = tail_probe(s, srp, sci, sv, tk, tail_ok);
      s->upa.bytes += 20.0 * (double)srp[tk];
      cuadmm_aat_tail_schur_release(s->fac);
      if (rc && rc != CUADMM_ERR_FACTOR) return (rc);
      if (!tail_ok) {
        set_error("update_A: the GPU tail of %d columns fails its factorisation or its probe solve on the new values (an init would fall back to the host-only factor)", tk);
        return (CUADMM_ERR_FACTOR);
      }
      if (s->world > 1 && !s->local_mode && s->sw.tail_shard != 0 && !s->sw.tail_refine && (rc = s->tail.keep_shard(s->rank, s->world, s->st))) return (rc);
    }
    // --- where the y-solve runs: init's stage again (the streams of the leading sweeps, the tree tops' inverses, L21), and its decisions
    if (s->tail.k > 0 && !s->sw.host_solve) {
      const bool o_dev = s->dev_solve, o_ready = s->lead.ready, o_tops = s->lead.tops, o_hyb = s->lead.hybrid;
      if ((rc = init_solve_plan(s, in, ctx))) return (rc);
      if (o_dev != s->dev_solve || o_ready != s->lead.ready || o_tops != s->lead.tops || o_hyb != s->lead.hybrid) {
        set_error("update_A: with the new values the y-solve would be planned differently (device %d -> %d, sweeps %d -> %d, tree tops %d -> %d, hybrid %d -> %d); only an init builds another plan",
                  (int)o_dev, (int)s->dev_solve, (int)o_ready, (int)s->lead.ready, (int)o_tops, (int)s->lead.tops, (int)o_hyb, (int)s->lead.hybrid);
        return (CUADMM_ERR_FACTOR);
      }
    } else if (s->forest_trees > 0) {
      const int64_t* Lp; const int* Li; const double* Lx; const double* D;
      if ((rc = cuadmm_aat_factor_arrays(s->fac, &Lp, &Li, &Lx, &D))) return (rc);
      if ((rc = s->f_Lx.upload(Lx, (size_t)Lp[m])) || (rc = s->f_D.upload(D, (size_t)m))) return (rc);
      s->upa.bytes += 8.0 * ((double)Lp[m] + (double)m);
    }
    if (inject == 2) { set_error("update_A: injected failure behind the rebuilt y-solve (test hook)"); return CUADMM_ERR_FACTOR; }
    return CUADMM_OK;
  };
  rc = factor_stage();
  if (s->local_mode && s->comm_world > 1) {
    // owned constraints: every rank factors its own A A^T.  The ranks agree on the outcome before the residual stage's collectives: one
    // rank that failed fails the call on all of them
    double bad[1] = {rc ? 1.0 : 0.0};
    int rc2 = s->allreduce_scalars(bad, 1);
    if (!rc && rc2) rc = rc2;
    if (!rc && bad[0] > 0) { set_error("update_A: another rank could not factor its share of the new A A^T"); rc = CUADMM_ERR_FACTOR; }
  }
  if (rc) return fail(rc);
  const double t_f2 = wall_s();

  // --- the value arrays of A and A^T: the maps at the first update, then one upload and one kernel
  if (!s->upa.maps) {
    auto& u = s->upa;
    const int* cp = u.cp.data();
    const int* ri = u.ri.data();
    // A^T by svec rows: slot q of the rank's share <- caller's position (the fill order of init_normalise)
    std::vector<int> from_rows((size_t)At_nnz);
    {
      std::vector<int> pos(ctx.rp.begin(), ctx.rp.end() - 1);
      for (int j = 0; j < m; ++j)
        for (int p = cp[j]; p < cp[j + 1]; ++p) from_rows[(size_t)pos[ri[p]]++] = p;
    }
    const int base = ctx.rp[s->sv_begin], cnt = ctx.rp[s->sv_end] - base;
    u.h_fromAt.assign(from_rows.begin() + base, from_rows.begin() + base + cnt);
    // A by permuted rows, local columns (the fill order of init_matrices)
    u.h_fromA.clear(); u.h_fromA.reserve((size_t)cnt);
    u.h_arp.assign((size_t)m + 1, 0);
    for (int pidx = 0; pidx < m; ++pidx) {
      const int j = s->perm[pidx];
      for (int p = cp[j]; p < cp[j + 1]; ++p)
        if (ri[p] >= s->sv_begin && ri[p] < s->sv_end) u.h_fromA.push_back(p);
      u.h_arp[(size_t)pidx + 1] = (int)u.h_fromA.size();
    }
    if (u.h_fromA.size() != s->A_v.n || (size_t)cnt != s->At_v.n) { set_error("update_A: the index maps do not match the device matrices"); return fail(CUADMM_ERR_INTERNAL); }
    if ((rc = u.fromA.from(u.h_fromA)) || (rc = u.fromAt.from(u.h_fromAt)) || (rc = u.src.alloc(std::max(At_nnz, 1)))) return fail(rc);
    u.maps = true;
  }
  if ((rc = s->upa.src.upload(ctx.vals.data(), (size_t)At_nnz))) return fail(rc);
  const bool timed = s->profile == 1;
  if (timed) for (auto& e : s->upa.ev) if (!e) CUADMM_HIP_TRY(hipEventCreate(&e));
  if (timed) CUADMM_HIP_TRY(hipEventRecord(s->upa.ev[0], s->st));      // the kernel alone: the upload above is a blocking copy of its own
  if ((rc = launch_gather_vals(s->A_v.p, s->upa.fromA.p, (long long)s->upa.h_fromA.size(), s->At_v.p, s->upa.fromAt.p, (long long)s->upa.h_fromAt.size(), s->upa.src.p, s->st)))
    return fail(rc);
  if (timed) CUADMM_HIP_TRY(hipEventRecord(s->upa.ev[1], s->st));
  s->upa.pass_bytes[0] = 20.0 * ((double)s->upa.h_fromA.size() + (double)s->upa.h_fromAt.size());      // per slot: 4 of map, 8 gathered, 8 stored
  s->upa.bytes += 8.0 * At_nnz;
  if (s->lrows.active) {
    // the rows evaluated inside the fused blocks' kernels keep copies of their values (and the compact matrix of the others its own)
    auto& lr = s->lrows;
    const auto& arp = s->upa.h_arp;
    const auto& fA = s->upa.h_fromA;
    std::vector<char> local((size_t)m, 0);
    size_t z = 0;
    for (int q = 0; q < lr.nlocal; ++q) {
      const int r = lr.h_row[q];
      local[r] = 1;
      for (int p = arp[r]; p < arp[r + 1]; ++p) lr.h_v[z++] = ctx.vals[fA[p]];
    }
    if ((rc = lr.v.upload(lr.h_v.data(), lr.h_v.size()))) return fail(rc);
    s->upa.bytes += 8.0 * (double)lr.h_v.size();
    if (lr.nrest > 0) {
      std::vector<double> rv2;
      for (int r = 0; r < m; ++r) {
        if (local[r]) continue;
        for (int p = arp[r]; p < arp[r + 1]; ++p) rv2.push_back(ctx.vals[fA[p]]);
      }
      if ((rc = lr.rest_v.upload(rv2.data(), rv2.size()))) return fail(rc);
      s->upa.bytes += 8.0 * (double)rv2.size();
    }
  }

  // --- scaling constants, b, and the iterate in the new units (init_vectors; b and C themselves are the caller's of before)
  double ibs = 1, ics = 1;
  {
    std::vector<double> bfull;
    const double nb2 = scaled_b(s->upa.b_idx.data(), s->upa.b_val.data(), (int)s->upa.b_idx.size(), nullptr, s->normA, bfull);
    s->set_scaled_b(bfull, s->local_mode ? s->ov_nb2 : nb2);
    s->objscale = s->bscale * s->Cscale;
    ibs = 1 / s->bscale; ics = 1 / s->Cscale;
    for (int pidx = 0; pidx < m; ++pidx) s->normA_p[pidx] = s->normA[s->perm[pidx]];
    if (s->b_d.p) {
      if ((rc = s->b_d.upload(s->b_p.data(), (size_t)m)) || (rc = s->normA_d.upload(s->normA_p.data(), (size_t)m))) return fail(rc);
      s->upa.bytes += 16.0 * (double)m;
    }
  }
  // --- closed blocks: init's routine, into the records of init
  if (s->closed.active) {
    if ((rc = init_closed(s, in, ctx))) return fail(rc);
    if (!s->closed.active) { set_error("update_A: the closed-block records could not be rebuilt on the new factor"); return fail(CUADMM_ERR_FACTOR); }
  }
  // (the iterate last: a call that failed above has left X, y, S in the caller's units, where a later update finds them)
  for (int pidx = 0; pidx < m; ++pidx) s->y_p[pidx] = keep ? (s->y_p[pidx] * s->normA_p[pidx]) * ics : 0.0;
  if (timed) CUADMM_HIP_TRY(hipEventRecord(s->upa.ev[2], s->st));
  if ((rc = launch_update_svec(s->X.p, s->S.p, nullptr, L, !keep, 1.0, ibs, 1.0, ics, s->st))) return fail(rc);
  if (timed) CUADMM_HIP_TRY(hipEventRecord(s->upa.ev[3], s->st));
  s->upa.pass_bytes[1] = (keep ? 32.0 : 16.0) * (double)L;
  if (sig > 0) s->sig = sig;
  s->factor_bad = false;
  if ((rc = s->reset_solve_state(t_begin))) return rc;
  s->y_host_stale = false;              // (materialise above left both as they are set here)
  s->pending_unscale = false;
  s->upa.bytes += 8.0 * (double)m;                             // y, uploaded by the residual stage

  rc = init_residuals(s, false);                               // (ends with a stream synchronisation)
  s->upa.pass_ms[0] = s->upa.pass_ms[1] = 0;
  if (timed && !rc)
    for (int q = 0; q < 2; ++q) s->upa.pass_ms[q] = event_ms(s->upa.ev[2 * q], s->upa.ev[2 * q + 1]);
  s->upa.count++;
  s->upa.host_ms = (t_f1 - t_f0) * 1e3;
  s->upa.dev_ms = (t_f2 - t_f1) * 1e3;
  s->upa.wall_ms = (wall_s() - t_begin) * 1e3;
  return rc;
}

int cuadmm_get_update_info(const cuadmm_solver* s, double o[6]) {
  if (!s || !o) { set_error("get_update_info: null"); return CUADMM_ERR_INVALID; }
  o[0] = (double)s->upa.count; o[1] = s->upa.wall_ms; o[2] = s->upa.host_ms; o[3] = s->upa.dev_ms; o[4] = (double)s->upa.orderings; o[5] = s->upa.bytes;
  return CUADMM_OK;
}

int cuadmm_get_update_pass_info(const cuadmm_solver* s, double o[4]) {
  if (!s || !o) { set_error("get_update_pass_info: null"); return CUADMM_ERR_INVALID; }
  o[0] = s->upa.pass_ms[0]; o[1] = s->upa.pass_bytes[0]; o[2] = s->upa.pass_ms[1]; o[3] = s->upa.pass_bytes[1];
  return CUADMM_OK;
}

int cuadmm_get_device_ptrs(cuadmm_solver* s, double** X, double** y, double** S) {
  if (!s || !s->initialised) { set_error("get_device_ptrs: not initialised"); return CUADMM_ERR_INVALID; }
  { int rc = s->materialise(); if (rc) return rc; }
  if (X) *X = s->X.p;
  if (y) *y = s->y_d.p;
  if (S) *S = s->S.p;
  return CUADMM_OK;
}

int cuadmm_get_shard(const cuadmm_solver* s, int64_t* b, int64_t* e, int* kb, int* ke) {
  if (!s || !s->initialised) { set_error("get_shard: not initialised"); return CUADMM_ERR_INVALID; }
  if (s->group && !s->in_group_call) {      // the leader's getters return whole vectors
    if (b) *b = 0;
    if (e) *e = s->local_mode ? s->L_caller : s->L_full;
    if (kb) *kb = 0;
    if (ke) *ke = s->local_mode ? s->nblk_caller : s->nblk_full;
    return CUADMM_OK;
  }
  if (b) *b = s->sv_off + s->sv_begin;
  if (e) *e = s->sv_off + s->sv_end;
  if (kb) *kb = s->blk_off + s->blk_begin;
  if (ke) *ke = s->blk_off + s->blk_end;
  return CUADMM_OK;
}

int cuadmm_get_info_iter_num(const cuadmm_solver* s) { return s ? s->info_iter_num : 0; }
int cuadmm_get_info_array(const cuadmm_solver* s, int which, double* out, int cap) {
  if (!s || which < 0 || which >= 8 || !out) { set_error("get_info_array: bad arguments"); return CUADMM_ERR_INVALID; }
  // the reference appends across solve() calls (vectors are never cleared, solver.cu:802-809)
  int n = std::min<int>(cap, (int)s->info[which].size());
  std::copy(s->info[which].begin(), s->info[which].begin() + n, out);
  return n;
}
double cuadmm_get_total_time(const cuadmm_solver* s) { return s ? s->total_time : 0.0; }
int cuadmm_get_state(const cuadmm_solver* s, double o[12]) {
  if (!s || !o) { set_error("get_state: null"); return CUADMM_ERR_INVALID; }
  o[0] = s->errRp; o[1] = s->errRd; o[2] = s->pobj; o[3] = s->dobj; o[4] = s->relgap; o[5] = s->sig;
  o[6] = s->bscale; o[7] = s->Cscale; o[8] = s->norm_borg; o[9] = s->norm_Corg; o[10] = s->best_KKT;
  o[11] = (double)s->eig_fail_total;
  return CUADMM_OK;
}

int cuadmm_get_profile(const cuadmm_solver* s, double out[3 * CUADMM_NUM_KCLASS]) {
  if (!s || !out) { set_error("get_profile: null"); return CUADMM_ERR_INVALID; }
  for (int k = 0; k < K_NUM; ++k) { out[3 * k] = s->prof_count[k]; out[3 * k + 1] = s->prof_ms[k]; out[3 * k + 2] = s->prof_bytes[k]; }
  return CUADMM_OK;
}
int cuadmm_get_psd_steps(cuadmm_solver* s, int* out, int cap) {
  if (!s || !out) { set_error("get_psd_steps: null"); return CUADMM_ERR_INVALID; }
  if (!s->steps_d.p && s->psd_steps && s->initialised && s->blk_local.empty()) return 0;     // a rank without blocks (PlanarHand_N=1 on eight ranks: its
                                                                                            // n = 120 block alone outweighs a rank's share) has nothing to report
  if (!s->steps_d.p) { set_error("get_psd_steps: set option psd_steps=1 before init"); return CUADMM_ERR_INVALID; }
  const int n = (int)std::min<size_t>(s->steps_d.n, (size_t)std::max(cap, 0));
  CUADMM_HIP_TRY(hipStreamSynchronize(s->st));
  { int rc2 = staged_d2h(out, s->steps_d.p, sizeof(int) * (size_t)n, s->st); if (rc2) return rc2; }
  return n;
}
int cuadmm_get_counters(const cuadmm_solver* s, double o[8]) {
  if (!s || !o) { set_error("get_counters: null"); return CUADMM_ERR_INVALID; }
  o[0] = (double)s->bt.launches; o[1] = (double)s->bt.iters; o[2] = (double)s->bt.rollbacks; o[3] = (double)cuadmm_host_pool_threads();
  o[4] = s->fuse ? 1 : 0; o[5] = s->closed.active ? 1 : 0; o[6] = s->dev_solve ? (s->lead.tops ? 3 : 1) : (s->lead.hybrid ? 2 : 0); o[7] = (double)s->tail.k;
  return CUADMM_OK;
}
int cuadmm_get_accel_info(const cuadmm_solver* s, double o[8]) {
  if (!s || !o) { set_error("get_accel_info: null"); return CUADMM_ERR_INVALID; }
  o[0] = (double)s->aa.mem; o[1] = (double)s->aa.taken; o[2] = (double)s->aa.accepted; o[3] = (double)s->aa.rejected; o[4] = (double)s->aa.restarts;
  o[5] = (double)s->aa.cols; o[6] = s->profile ? s->aa.ms : 0.0; o[7] = (double)(s->aa.ring_dF.n + s->aa.ring_dG.n) * sizeof(double);
  return CUADMM_OK;
}
int cuadmm_accel_solve_ls(const double* gram, const double* rhs, int cols, double reg, double* gamma_out) {
  return accel_solve_ls(gram, rhs, cols, reg, gamma_out);
}
int cuadmm_get_status(const cuadmm_solver* s, double o[8]) {
  if (!s || !o) { set_error("get_status: null"); return CUADMM_ERR_INVALID; }
  o[0] = (double)s->solve_status; o[1] = (double)s->solve_status_iter; o[2] = (double)s->inf.checks; o[3] = s->inf.scalar; o[4] = s->inf.eta;
  o[5] = s->inf.radius; o[6] = s->inf.ms; o[7] = s->inf.bytes() + (s->inf.xprev.p ? s->aux.bytes() : 0.0);
  return CUADMM_OK;
}
int cuadmm_get_certificate(cuadmm_solver* s, double* y_out, double* X_out) {
  if (!s || !s->initialised) { set_error("get_certificate: solver not initialised"); return CUADMM_ERR_INVALID; }
  if (s->solve_status != 3 && s->solve_status != 4) { set_error("get_certificate: the last solve found no certificate of infeasibility (status %d)", s->solve_status); return CUADMM_ERR_INVALID; }
  const std::vector<double>& c = s->inf.cert;
  if (s->solve_status == 3) {
    if (!y_out) { set_error("get_certificate: status 3 returns a y ray: y_out is null"); return CUADMM_ERR_INVALID; }
    // back to the caller's units and order as materialise / cuadmm_get_y map y, then b' y = 1 on the caller's b
    for (int i = 0; i < s->m; ++i) y_out[s->perm[i]] = c[i] / s->normA_p[i];
    long double t = 0;
    for (size_t k = 0; k < s->upa.b_idx.size(); ++k) t += (long double)s->upa.b_val[k] * y_out[s->upa.b_idx[k]];
    for (int i = 0; i < s->m; ++i) y_out[i] = (double)(y_out[i] / t);
    return CUADMM_OK;
  }
  if (!X_out) { set_error("get_certificate: status 4 returns an X ray: X_out is null"); return CUADMM_ERR_INVALID; }
  int rc = check_device(s->device);
  if (rc) return rc;
  std::vector<double> Ch((size_t)s->L);
  if (s->L > 0 && (rc = staged_d2h(Ch.data(), s->C.p, sizeof(double) * (size_t)s->L, s->st))) return rc;
  long double t = 0;
  for (long long i = 0; i < s->L; ++i) t += (long double)(Ch[i] * s->Cscale) * c[i];      // <C, dX> in the caller's units of C
  for (long long i = 0; i < s->L; ++i) X_out[i] = (double)(c[i] / -t);
  return CUADMM_OK;
}
int cuadmm_infeas_decide(const double stats[8], double tol, int* verdict, double* radius) {
  double o3[3];
  int rc = infeas_decide(stats, tol, verdict, o3);
  if (!rc && radius) *radius = o3[2];
  return rc;
}
int cuadmm_set_trace_bounds(cuadmm_solver* s, const double* R, int mat_num) {
  if (!s) { set_error("set_trace_bounds: null"); return CUADMM_ERR_INVALID; }
  if (!R) {
    if (s->initialised && s->lb.period > 0) { set_error("set_trace_bounds: option gap_check is on: the bounds cannot be cleared"); return CUADMM_ERR_INVALID; }
    s->lb.R.clear();
    return CUADMM_OK;
  }
  if (mat_num < 1) { set_error("set_trace_bounds: mat_num = %d", mat_num); return CUADMM_ERR_INVALID; }
  if (s->initialised) {
    int mn = 0;
    cuadmm_get_dims(s, nullptr, nullptr, &mn);
    if (mn != mat_num) { set_error("set_trace_bounds: %d bounds for a problem of %d blocks", mat_num, mn); return CUADMM_ERR_INVALID; }
  }
  for (int k = 0; k < mat_num; ++k)
    if (!(R[k] >= 0) || !std::isfinite(R[k])) { set_error("set_trace_bounds: bound %d is %g: every bound must be finite and not negative", k, R[k]); return CUADMM_ERR_INVALID; }
  s->lb.R.assign(R, R + mat_num);
  s->lb.R_dirty = true;
  return CUADMM_OK;
}
// What every report on a point refuses before it touches the device ("The front of the point reports").  what: the results that
// are not all-reduced; reads_A: the report reads A', C, b and the scaling constants, which a failed cuadmm_update_A leaves half updated.
static int report_guard(const cuadmm_solver* s, const void* out, const char* who, const char* what, bool reads_A) {
  if (!s || !s->initialised || !out) { set_error("%s: solver not initialised or null argument", who); return CUADMM_ERR_INVALID; }
  if (s->world > 1 || s->comm_world > 1 || s->local_mode || s->group || s->in_group_call) {
    set_error("%s: works on one rank (world = %d%s): its %s are not all-reduced", who, std::max(s->world, s->comm_world), s->group ? ", in-process group" : "", what);
    return CUADMM_ERR_INVALID;
  }
  if (s->L <= 0) { set_error("%s: the problem has no svec slots", who); return CUADMM_ERR_INVALID; }
  if (reads_A && s->factor_bad) { set_error("%s: the last cuadmm_update_A could not factor the new A A^T; the solver needs a successful cuadmm_update_A first", who); return CUADMM_ERR_FACTOR; }
  return check_device(s->device);
}
// Each report: the guard, its own checks, its vectors (*_prepare), the point staged in them, the run.
int cuadmm_lower_bound(cuadmm_solver* s, double o[8], double* per_block) {
  int rc = report_guard(s, o, "lower_bound", "sums", true);
  if (rc) return rc;
  if (s->lb.R.empty()) { set_error("lower_bound: no trace bounds are set (cuadmm_set_trace_bounds)"); return CUADMM_ERR_INVALID; }
  if ((rc = s->lb_prepare()) || (rc = s->stage_scaled_y(s->lb.ybuf.p, nullptr))) return rc;
  return s->lb_report(o, per_block);
}
int cuadmm_get_gap_info(const cuadmm_solver* s, double o[8]) {
  if (!s || !o) { set_error("get_gap_info: null"); return CUADMM_ERR_INVALID; }
  o[0] = (double)s->lb.checks; o[1] = s->lb.best_lb; o[2] = (double)s->lb.best_iter; o[3] = s->lb.last_lb; o[4] = s->lb.last_g;
  o[5] = s->lb.ms; o[6] = s->lb.bytes() + (s->lb.out_d.p ? s->btasks.bytes() + s->aux.bytes() : 0.0); o[7] = (double)s->lb.verdict_iter;
  return CUADMM_OK;
}
int cuadmm_evaluate(cuadmm_solver* s, const double* X, const double* y, const double* S, double o[16], double* per_block) {
  int rc = report_guard(s, o, "evaluate", "sums", true);
  if (rc) return rc;
  // before anything is uploaded: a passed vector with an entry that is not finite
  const struct { const char* name; const double* v; long long n; } in[3] = {{"X", X, s->L}, {"y", y, s->m}, {"S", S, s->L}};
  for (const auto& q : in)
    for (long long i = 0; q.v && i < q.n; ++i)
      if (!std::isfinite(q.v[i])) { set_error("evaluate: %s[%lld] is not finite", q.name, i); return CUADMM_ERR_INVALID; }
  if ((rc = s->ev_prepare())) return rc;
  // The point in the engine's scaled space and order, in vectors of the evaluation's own (the constants of materialise(), inverted, as
  // cuadmm_init and cuadmm_solve(if_first = 0) apply them).  A null vector is the one its getter would return: behind a solve the
  // iterate is held scaled and is read as it lies, otherwise it is in the caller's units (stage_scaled_y has the cases of y).
  const double *xs = nullptr, *ss = nullptr;
  if ((rc = s->ev_point(X, s->X, 1 / s->bscale, s->ev.xs, &xs)) || (rc = s->ev_point(S, s->S, 1 / s->Cscale, s->ev.ss, &ss)) ||
      (rc = s->stage_scaled_y(s->ev.cons.p, y)))
    return rc;
  return s->ev_run(xs, ss, o, per_block);
}
int cuadmm_lambda_min(cuadmm_solver* s, int which, int steps, double o[8], double* per_block) {
  int rc = report_guard(s, o, "lambda_min", "results", which == 2);
  if (rc) return rc;
  if (which < 0 || which > 2) { set_error("lambda_min: which = %d (0: X, 1: S, 2: C - A'y)", which); return CUADMM_ERR_INVALID; }
  if (steps < 1 || steps > kLmStepsMax) { set_error("lambda_min: steps = %d, allowed are 1 to %d", steps, kLmStepsMax); return CUADMM_ERR_INVALID; }
  if (which == 2 && !s->lb.R.empty() && s->lb.R.size() != s->blk_local.size()) {
    set_error("lambda_min: %d trace bounds are set, the solver has %d blocks", (int)s->lb.R.size(), (int)s->blk_local.size());
    return CUADMM_ERR_INVALID;
  }
  if ((rc = s->lm_prepare(which)) || (which == 2 && (rc = s->stage_scaled_y(s->lm.ybuf.p, nullptr)))) return rc;
  return s->lm_run(which, steps, o, per_block);
}
int cuadmm_lowrank_size(const cuadmm_solver* s, int rmax, long long* count_out) {
  if (!s || !s->initialised || !count_out) { set_error("lowrank_size: solver not initialised or null argument"); return CUADMM_ERR_INVALID; }
  if (rmax < 1 || rmax > kMaxBlockSize) { set_error("lowrank_size: rmax = %d, allowed are 1 to %d", rmax, kMaxBlockSize); return CUADMM_ERR_INVALID; }
  long long c = 0;
  for (int n : s->blk_local)
    if (n > 0) c += (long long)n * std::min(n, rmax);
  *count_out = c;
  return CUADMM_OK;
}
int cuadmm_lowrank(cuadmm_solver* s, int which, double tol, int rmax, double o[8], double* per_block, double* L_out, int* piv_out) {
  int rc = report_guard(s, o, "lowrank", "results", false);
  if (rc) return rc;
  if (which < 0 || which > 1) { set_error("lowrank: which = %d (0: X, 1: S)", which); return CUADMM_ERR_INVALID; }
  if (!(tol >= 0.0 && tol < 1.0)) { set_error("lowrank: tol = %g, allowed is 0 <= tol < 1", tol); return CUADMM_ERR_INVALID; }
  if (rmax < 1 || rmax > kMaxBlockSize) { set_error("lowrank: rmax = %d, allowed are 1 to %d", rmax, kMaxBlockSize); return CUADMM_ERR_INVALID; }
  if ((rc = s->lr_prepare(rmax))) return rc;
  return s->lr_run(which, tol, o, per_block, L_out, piv_out);
}
int cuadmm_get_evaluate_info(const cuadmm_solver* s, double o[4]) {
  if (!s || !o) { set_error("get_evaluate_info: null"); return CUADMM_ERR_INVALID; }
  o[0] = (double)s->ev.calls; o[1] = s->ev.bytes() + (s->ev.out_d.p ? s->btasks.bytes() : 0.0); o[2] = s->ev.out_d.p ? s->aux.bytes() : 0.0; o[3] = s->ev.ms;
  return CUADMM_OK;
}
int cuadmm_trace_bounds_detect(int vec_len, int con_num, const int* At_csc_col_ptrs, const int* At_csc_row_ids, const double* At_csc_vals,
                               const int* b_indices, const double* b_vals, int b_nnz, const int* blk_vals, int mat_num, double* R_out) {
  return lb_trace_bounds_detect(vec_len, con_num, At_csc_col_ptrs, At_csc_row_ids, At_csc_vals, b_indices, b_vals, b_nnz, blk_vals, mat_num, R_out);
}
int cuadmm_get_tail_info(const cuadmm_solver* s, double o[6]) {
  if (!s || !o) { set_error("get_tail_info: null"); return CUADMM_ERR_INVALID; }
  o[0] = (double)s->tail.k; o[1] = s->tail.shard_bytes; o[2] = (double)s->tail.shard_rows; o[3] = s->tail.resident_bytes;
  o[4] = s->tail.inv_resid; o[5] = (s->tail.refine && s->tail.Lm) ? 1.0 : 0.0;
  return CUADMM_OK;
}
int cuadmm_get_group_info(const cuadmm_solver* s, double o[4]) {
  if (!s || !o) { set_error("get_group_info: null"); return CUADMM_ERR_INVALID; }
  o[0] = s->group ? (double)duo_group_world(s->group) : 1.0;
  o[1] = s->group ? (double)duo_group_exchange(s->group) : 0.0;
  o[2] = s->group ? (double)duo_group_distinct_devices(s->group) : 1.0;
  o[3] = s->group ? (double)duo_group_allreduces(s->group) : 0.0;
  return CUADMM_OK;
}
int cuadmm_reset_profile(cuadmm_solver* s) {
  if (!s) { set_error("reset_profile: null"); return CUADMM_ERR_INVALID; }
  for (int k = 0; k < K_NUM; ++k) { s->prof_count[k] = 0; s->prof_ms[k] = 0; }
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// op-level entry points that need the planner
// ------------------------------------------------------------------------------------------
int cuadmm_op_batch_eig(double* mat, double* W, int* info, int n, int count, void* stream) {
  return psd_batch_eig(mat, W, info, n, count, (hipStream_t)stream);
}

int cuadmm_op_gemm_sym(int n, const double* A, const double* B, double alpha, double beta, const double* E, double* Cout, void* stream) {
  if (n < 64 || n % 64 != 0 || !A || !B || !Cout) { set_error("gemm_sym: n must be a positive multiple of 64 and pointers non-null"); return CUADMM_ERR_INVALID; }
  return large_gemm_sym(n, A, B, alpha, beta, E, Cout, (hipStream_t)stream);
}

int cuadmm_op_tail_factor_solve(const int64_t* row_ptr, const int* col, const double* val, int k, double* z_host, int nrhs) {
  if (!row_ptr || !col || !val || !z_host || k < 1 || nrhs < 0) { set_error("tail_factor_solve: bad arguments"); return CUADMM_ERR_INVALID; }
  TailSolve t;
  int rc = t.build_from_schur(reinterpret_cast<const long long*>(row_ptr), col, val, k, nullptr);
  for (int r = 0; r < nrhs && !rc; ++r) rc = t.solve(z_host + (size_t)r * k, nullptr);
  return rc;
}

int cuadmm_op_tail_solve(const double* L22_host, const double* D2_host, int k, double* z2_host, int nrhs) {
  if (!L22_host || !D2_host || !z2_host || k < 1 || nrhs < 0) { set_error("tail_solve: bad arguments"); return CUADMM_ERR_INVALID; }
  TailSolve t;
  int rc = t.build(L22_host, D2_host, k, nullptr);
  for (int r = 0; r < nrhs && !rc; ++r) rc = t.solve(z2_host + (size_t)r * k, nullptr);
  if (!rc) {
    const int lost = t.fail_count(nullptr);
    if (lost != 0) { set_error("tail_solve: %d row exchanges lost (workgroups of a row not co-resident)", lost); return CUADMM_ERR_FACTOR; }
  }
  return rc;
}

int cuadmm_op_tail_solve_sharded(const double* L22_host, const double* D2_host, int k, const double* z_host, int world, int one_pass,
                                 double* out_host, int* rows_out) {
  if (!L22_host || !D2_host || !z_host || !out_host || k < 1 || world < 1) { set_error("tail_solve_sharded: bad arguments"); return CUADMM_ERR_INVALID; }
  const bool compact = (one_pass & 2) != 0;      // + 2: every rank KEEPS its rows only (TailSolve::keep_shard), one object per rank
  int rc = CUADMM_OK;
  for (int p = 0; p < world && !rc; ++p) {
    TailSolve t;
    t.one_pass = (one_pass & 1) != 0;
    if ((rc = t.build(L22_host, D2_host, k, nullptr))) break;
    // the reduction is left out: every rank's partial result comes back as it stands
    t.reduce_fn = [](void*, double*, size_t, hipStream_t) -> int { return CUADMM_OK; };
    t.shard_world = world;
    const int p_end = compact ? p + 1 : world;   // without compaction ONE object serves every rank in turn
    for (int q = p; q < p_end && !rc; ++q) {
      t.shard_rank = q;
      if (compact && (rc = t.keep_shard(q, world, nullptr))) break;
      std::copy(z_host, z_host + k, out_host + (size_t)q * k);
      rc = t.solve(out_host + (size_t)q * k, nullptr);
      if (rows_out) rows_out[q] = t.shard_rows;
    }
    if (!rc) {
      const int lost = t.fail_count(nullptr);
      if (lost != 0) { set_error("tail_solve_sharded: %d row exchanges lost", lost); return CUADMM_ERR_FACTOR; }
    }
    if (!compact) break;
  }
  return rc;
}

// Failure drill of the four-workgroups-per-row tail kernel (18 432 < K <= 32 768), see the protocol above ts_onepass_group_kernel:
// out[0] = the plain solve of z; out[1] = the solve of z with a NaN carrying the exchange sentinel's bits in z[0] (must come back as
// NaN promptly, no exchange lost: counts[0] = 0); out[2] = the solve with the failure counter raised beforehand (NaN at once,
// counts[1] = the count take_failure() found and cleared); out[3] = the solve after that, on the two-GEMV path the object retired to
// (counts[2] = 1).  Test hook only.
int cuadmm_op_tail_solve_drill(const double* L22_host, const double* D2_host, int k, const double* z_host, double* out_host, int* counts) {
  if (!L22_host || !D2_host || !z_host || !out_host || !counts || k < 1) { set_error("tail_solve_drill: bad arguments"); return CUADMM_ERR_INVALID; }
  TailSolve t;
  int rc = t.build(L22_host, D2_host, k, nullptr);
  if (rc) return rc;
  if (!t.d_fail) { set_error("tail_solve_drill: k = %d does not use the row-sharing kernel", k); return CUADMM_ERR_INVALID; }
  for (int q = 0; q < 4; ++q) std::copy(z_host, z_host + k, out_host + (size_t)q * k);
  if ((rc = t.solve(out_host, nullptr))) return rc;
  { const unsigned long long bits = 0x7ff8dead5eed0001ull; std::memcpy(out_host + (size_t)k, &bits, sizeof bits); }
  if ((rc = t.solve(out_host + (size_t)k, nullptr))) return rc;
  counts[0] = t.fail_count(nullptr);
  CUADMM_HIP_TRY(hipMemset(t.d_fail, 0, sizeof(int)));
  { const int one = 1; CUADMM_HIP_TRY(hipMemcpy(t.d_fail, &one, sizeof one, hipMemcpyHostToDevice)); }
  if ((rc = t.solve(out_host + 2 * (size_t)k, nullptr))) return rc;
  counts[1] = t.take_failure(nullptr);
  counts[2] = t.group_retired ? 1 : 0;
  return t.solve(out_host + 3 * (size_t)k, nullptr);
}

// Test hook only: the device y-solve around the GPU tail on its own.  The tail and the leading sweeps are built from the split factor the
// way init_factor / init_solve_plan build them (the tail from the Schur complement with the engine's default switches; LeadSolve with the
// switches given), and whatever build() made ready runs -- the engine's cost-model veto (est_us against the host's sweeps) is NOT applied.
// force_hybrid: the engine's hybrid sequence (host sweeps over L11, apply_l21 between them), demoting ready sweeps if need be.
// ax / asmc / b: nrhs x m (factor's order), y_out likewise; one pair of objects serves all right-hand sides in turn.  y is filled with NaN
// before every solve, so a row no kernel wrote comes back as NaN.  The factor keeps its Schur complement (the caller may read it).
// info11 = {ntrees, max_levels, n_small, n_big, n_stream, n_micro, n_long, tops, nT, hybrid, ready}.
int cuadmm_op_lead_solve(const cuadmm_aat* f, int m, int stream_only, int small_kb, int tops_level, int force_hybrid, const double* ax,
                         const double* asmc, const double* b, double isig, int nrhs, double* y_out, int* info11) {
  if (!f || m < 1 || !ax || !asmc || !b || !y_out || !info11 || nrhs < 0) { set_error("op_lead_solve: bad arguments"); return CUADMM_ERR_INVALID; }
  const int k = cuadmm_aat_tail_k(f);
  if (k < 1 || k > m) { set_error("op_lead_solve: a split factor of %d rows (tail %d)", m, k); return CUADMM_ERR_INVALID; }
  const int64_t *srp, *Lp; const int *sci, *Li; const double *sv, *Lx, *D;
  int rc;
  if ((rc = cuadmm_aat_tail_schur(f, &srp, &sci, &sv)) || (rc = cuadmm_aat_factor_arrays(f, &Lp, &Li, &Lx, &D))) return rc;
  TailSolve tail;
  if ((rc = tail.build_from_schur(reinterpret_cast<const long long*>(srp), sci, sv, k, nullptr))) return rc;
  LeadSolve lead;
  lead.stream_only = stream_only != 0;
  lead.force_hybrid = force_hybrid != 0;
  lead.small_kb = std::max(0, std::min(small_kb, 36));
  lead.tops_level = force_hybrid ? 0 : tops_level;
  if ((rc = lead.build(m, k, Lp, Li, Lx, D, true))) return rc;
  if (force_hybrid && !lead.hybrid && !(lead.ready && lead.demote_to_hybrid())) { set_error("op_lead_solve: no hybrid solve for this factor"); return CUADMM_ERR_INVALID; }
  if (!lead.ready && !lead.hybrid) { set_error("op_lead_solve: neither the device sweeps nor the hybrid solve could be built"); return CUADMM_ERR_INVALID; }
  const int info[11] = {lead.ntrees, lead.max_levels, lead.n_small, lead.n_big, lead.n_stream, lead.n_micro, lead.n_long, lead.tops ? 1 : 0, lead.nT,
                        lead.hybrid ? 1 : 0, lead.ready ? 1 : 0};
  std::copy(info, info + 11, info11);
  DevBuf<double> ax_d, asmc_d, b_d, y_d;
  if ((rc = ax_d.alloc(m)) || (rc = asmc_d.alloc(m)) || (rc = b_d.alloc(m)) || (rc = y_d.alloc(m))) return rc;
  std::vector<double> yh((size_t)m);
  for (int r = 0; r < nrhs; ++r) {
    const double *axr = ax + (size_t)r * m, *asr = asmc + (size_t)r * m, *br = b + (size_t)r * m;
    double* yr = y_out + (size_t)r * m;
    if (lead.hybrid) {
      for (int i = 0; i < m; ++i) yh[i] = -asr[i] + isig * (-axr[i] + br[i]);       // host_solve()'s right-hand side
      if ((rc = cuadmm_aat_solve_leading_forward11(f, k, yh.data())) || (rc = lead.apply_l21(yh.data(), false, tail, nullptr)) ||
          (rc = cuadmm_aat_solve_leading_backward11(f, k, yh.data(), lead.h_w)))
        return rc;
      std::copy(yh.begin(), yh.end(), yr);
    } else {
      if ((rc = ax_d.upload(axr, m)) || (rc = asmc_d.upload(asr, m)) || (rc = b_d.upload(br, m))) return rc;
      CUADMM_HIP_TRY(hipMemset(y_d.p, 0xff, sizeof(double) * (size_t)m));
      if ((rc = lead.solve(ax_d.p, asmc_d.p, b_d.p, isig, y_d.p, tail, nullptr))) return rc;
      CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
      if ((rc = staged_d2h(yr, y_d.p, sizeof(double) * (size_t)m))) return rc;
    }
  }
  const int lost = tail.fail_count(nullptr);
  if (lost != 0) { set_error("op_lead_solve: %d row exchanges of the tail lost", lost); return CUADMM_ERR_FACTOR; }
  return CUADMM_OK;
}

// Test hook only: one thread per tree of a one-piece factor's elimination forest (forest_solve_kernel), with the arrays the engine uploads
// in init_solve_plan.  info2 = {trees, columns of the largest tree}.
int cuadmm_op_forest_solve(cuadmm_aat* f, int m, const double* ax, const double* asmc, const double* b, double isig, double* y_out, int* info2) {
  if (!f || m < 1 || !ax || !asmc || !b || !y_out || !info2) { set_error("op_forest_solve: bad arguments"); return CUADMM_ERR_INVALID; }
  if (cuadmm_aat_tail_k(f) != 0) { set_error("op_forest_solve: a one-piece factor"); return CUADMM_ERR_INVALID; }
  int ntrees = 0, maxc = 0, rc;
  const int *tp = nullptr, *tc = nullptr;
  const int64_t* Lp; const int* Li; const double* Lx; const double* D;
  if ((rc = cuadmm_aat_forest(f, &ntrees, &maxc, &tp, &tc)) || (rc = cuadmm_aat_factor_arrays(f, &Lp, &Li, &Lx, &D))) return rc;
  const size_t lnz = (size_t)Lp[m];
  DevBuf<int> d_tp, d_tc, d_Li;
  DevBuf<long long> d_Lp;
  DevBuf<double> d_Lx, d_D, ax_d, asmc_d, b_d, y_d;
  if ((rc = d_tp.from(std::vector<int>(tp, tp + ntrees + 1))) || (rc = d_tc.from(std::vector<int>(tc, tc + m))) ||
      (rc = d_Lp.from(std::vector<long long>(Lp, Lp + m + 1))) || (rc = d_Li.from(std::vector<int>(Li, Li + lnz))) ||
      (rc = d_Lx.from(std::vector<double>(Lx, Lx + lnz))) || (rc = d_D.from(std::vector<double>(D, D + m))) ||
      (rc = ax_d.from(std::vector<double>(ax, ax + m))) || (rc = asmc_d.from(std::vector<double>(asmc, asmc + m))) ||
      (rc = b_d.from(std::vector<double>(b, b + m))) || (rc = y_d.alloc(m)))
    return rc;
  CUADMM_HIP_TRY(hipMemset(y_d.p, 0xff, sizeof(double) * (size_t)m));
  if ((rc = launch_forest_solve(ntrees, d_tp.p, d_tc.p, d_Lp.p, d_Li.p, d_Lx.p, d_D.p, ax_d.p, asmc_d.p, b_d.p, isig, y_d.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  info2[0] = ntrees; info2[1] = maxc;
  return staged_d2h(y_out, y_d.p, sizeof(double) * (size_t)m);
}

// op-level hook of the value pass of cuadmm_update_A: outA[offA + q] = src[fromA[q]], outAt[offAt + q] = src[fromAt[q]]; the targets are
// device arrays of nA + offA + 2 (nAt + offAt + 2) doubles filled with `fill` first, returned whole (what the kernel must leave alone included)
int cuadmm_op_gather_vals(const double* src, int n_src, const int* fromA, int nA, int offA, const int* fromAt, int nAt, int offAt, double fill,
                          double* outA, double* outAt) {
  if (!src || n_src < 1 || nA < 0 || nAt < 0 || offA < 0 || offAt < 0 || (nA > 0 && !fromA) || (nAt > 0 && !fromAt) || !outA || !outAt) { set_error("op_gather_vals: bad arguments"); return CUADMM_ERR_INVALID; }
  for (int q = 0; q < nA; ++q) if (fromA[q] < 0 || fromA[q] >= n_src) { set_error("op_gather_vals: index out of range"); return CUADMM_ERR_INVALID; }
  for (int q = 0; q < nAt; ++q) if (fromAt[q] < 0 || fromAt[q] >= n_src) { set_error("op_gather_vals: index out of range"); return CUADMM_ERR_INVALID; }
  int rc;
  DevBuf<double> d_src, dA, dAt;
  DevBuf<int> d_fA, d_fAt;
  const size_t lenA = (size_t)nA + offA + 2, lenAt = (size_t)nAt + offAt + 2;
  std::vector<double> hA(lenA, fill), hAt(lenAt, fill);
  if ((rc = d_src.from(std::vector<double>(src, src + n_src))) || (rc = dA.from(hA)) || (rc = dAt.from(hAt)) ||
      (rc = d_fA.from(std::vector<int>(fromA, fromA + nA))) || (rc = d_fAt.from(std::vector<int>(fromAt, fromAt + nAt))))
    return rc;
  if ((rc = launch_gather_vals(dA.p + offA, d_fA.p, nA, dAt.p + offAt, d_fAt.p, nAt, d_src.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipDeviceSynchronize());
  if ((rc = staged_d2h(outA, dA.p, sizeof(double) * lenA)) || (rc = staged_d2h(outAt, dAt.p, sizeof(double) * lenAt))) return rc;
  return CUADMM_OK;
}

int cuadmm_op_psd_project(const double* Xb, double* Xproj, const int* blk_host, int mat_num, void* stream) {
  return cuadmm_op_psd_project_steps(Xb, Xproj, blk_host, mat_num, nullptr, stream);
}

int cuadmm_op_psd_project_steps(const double* Xb, double* Xproj, const int* blk_host, int mat_num, int* steps_dev, void* stream) {
  return cuadmm_op_psd_project_ex(Xb, Xproj, blk_host, mat_num, 0, steps_dev, stream);
}

int cuadmm_op_psd_project_ex(const double* Xb, double* Xproj, const int* blk_host, int mat_num, int eig_rank, int* steps_dev, void* stream) {
  if (!blk_host || mat_num < 0 || eig_rank < 0) { set_error("psd_project: bad arguments"); return CUADMM_ERR_INVALID; }
  PsdPlan plan;
  plan.eig_rank = eig_rank;
  int rc = plan.build(blk_host, mat_num);
  if (rc) return rc;
  if (steps_dev) {
    CUADMM_HIP_TRY(hipMemsetAsync(steps_dev, 0, sizeof(int) * (size_t)mat_num, (hipStream_t)stream));
    plan.d_steps = steps_dev;
    plan.sign.d_steps = steps_dev;
  }
  rc = plan.project(Xb, Xproj, (hipStream_t)stream);
  if (rc) return rc;
  int fails = plan.fail_count((hipStream_t)stream);   // synchronises the stream
  if (fails != 0) { set_error("psd_project: %d blocks hit the QL sweep cap", fails); return CUADMM_ERR_EIG; }
  return CUADMM_OK;
}

// own: the test hooks' non-blocking stream (cuadmm_psd_plan_project_ordered), made on first use
struct cuadmm_psd_plan {
  PsdPlan plan;
  hipStream_t own = nullptr;
  ~cuadmm_psd_plan() {
    if (own) { hipError_t e = hipStreamSynchronize(own); (void)e; e = hipStreamDestroy(own); (void)e; }   // idle before the plan's side streams and events go
  }
};
int cuadmm_psd_plan_create(const int* blk_host, int mat_num, int eig_rank, cuadmm_psd_plan** out) {
  if (!blk_host || mat_num < 0 || eig_rank < 0 || !out) { set_error("psd_plan_create: bad arguments"); return CUADMM_ERR_INVALID; }
  cuadmm_psd_plan* p = new cuadmm_psd_plan();
  p->plan.eig_rank = eig_rank;
  int rc = p->plan.build(blk_host, mat_num);
  if (rc) { delete p; return rc; }
  p->plan.overlap = true;
  *out = p;
  return CUADMM_OK;
}
int cuadmm_psd_plan_project(cuadmm_psd_plan* p, const double* Xb, double* Xproj, int* steps_dev, void* stream) {
  if (!p || !Xb || !Xproj) { set_error("psd_plan_project: bad arguments"); return CUADMM_ERR_INVALID; }
  p->plan.d_steps = steps_dev;
  p->plan.sign.d_steps = steps_dev;
  return p->plan.project(Xb, Xproj, (hipStream_t)stream);
}
void cuadmm_psd_plan_destroy(cuadmm_psd_plan* p) { delete p; }
int cuadmm_psd_plan_ranges(const int* blk_host, int mat_num, int eig_rank, int tiny_sign, const char* const* opt_keys, const double* opt_vals,
                           int n_opts, int* ranges_out, int* ids_out, int* slot_out, int* rest_out, int* summary_out) {
  if (!blk_host || mat_num < 0 || eig_rank < 0 || n_opts < 0 || !ranges_out || !ids_out || !slot_out || !rest_out || !summary_out) {
    set_error("psd_plan_ranges: bad arguments"); return CUADMM_ERR_INVALID;
  }
  PsdPlan plan;
  plan.opt = PsdOptions();
  for (int i = 0; i < n_opts; ++i)
    if (!plan.opt.set(opt_keys[i], opt_vals[i])) { set_error("psd_plan_ranges: unknown option %s", opt_keys[i]); return CUADMM_ERR_INVALID; }
  plan.eig_rank = eig_rank;
  plan.tiny_sign = tiny_sign != 0;
  int rc = plan.build_host(blk_host, mat_num);
  if (rc) return rc;
  for (const PsdRange& r : plan.ranges)
    for (int v : {r.cls, r.first, r.count, (int)r.kind, r.nt, r.occ, r.occ_batch, (int)r.full, (int)r.triple, r.maxn}) *ranges_out++ = v;
  std::vector<int> slot_of, rest;
  plan.fused_slots(slot_of);
  plan.rest_elements(rest);
  std::copy(plan.h_ids.begin(), plan.h_ids.end(), ids_out);
  std::copy(slot_of.begin(), slot_of.end(), slot_out);
  std::copy(rest.begin(), rest.end(), rest_out);
  const int summary[6] = {plan.ranges.n, (int)plan.h_ids.size(), (int)rest.size(), plan.fusable() ? 1 : 0, plan.fused_blocks(), plan.ranges.sign_min};
  std::copy(summary, summary + 6, summary_out);
  return CUADMM_OK;
}

// ---- the plan in the state the engine keeps it in (tests): schedule hints, re-sorted descriptors, a non-blocking caller's stream
static int psd_plan_stream(cuadmm_psd_plan* p, int own_stream, hipStream_t* st) {
  if (own_stream && !p->own) CUADMM_HIP_TRY(hipStreamCreateWithFlags(&p->own, hipStreamNonBlocking));
  *st = own_stream ? p->own : nullptr;
  return CUADMM_OK;
}
int cuadmm_psd_plan_set_hint(cuadmm_psd_plan* p, int* hint_dev, int hint_max_n) {
  if (!p) { set_error("psd_plan_set_hint: bad arguments"); return CUADMM_ERR_INVALID; }
  p->plan.d_hint = hint_dev;
  p->plan.sign.d_hint = hint_dev;
  p->plan.sign.hint_max_n = hint_max_n;
  return CUADMM_OK;
}
int cuadmm_psd_plan_reorder(cuadmm_psd_plan* p, const int* steps_host, int async, int own_stream) {
  if (!p || !steps_host) { set_error("psd_plan_reorder: bad arguments"); return CUADMM_ERR_INVALID; }
  hipStream_t st;
  int rc = psd_plan_stream(p, own_stream, &st);
  if (rc) return rc;
  return async ? p->plan.reorder_by_steps_async(steps_host, st) : p->plan.reorder_by_steps(steps_host, st);
}
int cuadmm_psd_plan_project_ordered(cuadmm_psd_plan* p, const double* Xb, double* Xproj, double* snap_dev, int* steps_dev, int own_stream, int* fails_out) {
  if (!p || !Xb || !Xproj) { set_error("psd_plan_project_ordered: bad arguments"); return CUADMM_ERR_INVALID; }
  hipStream_t st;
  int rc = psd_plan_stream(p, own_stream, &st);
  if (rc) return rc;
  p->plan.d_steps = steps_dev;
  p->plan.sign.d_steps = steps_dev;
  if ((rc = p->plan.project(Xb, Xproj, st))) return rc;
  // the snapshot is a consumer ordered by `st` alone: what a class that was not joined has not written yet is missing from it (a
  // device-wide synchronisation would wait for it); fail_count waits for `st` only
  if (snap_dev && p->plan.vec_len > 0)
    CUADMM_HIP_TRY(hipMemcpyAsync(snap_dev, Xproj, sizeof(double) * (size_t)p->plan.vec_len, hipMemcpyDeviceToDevice, st));
  const int fails = p->plan.fail_count(st);
  if (fails < 0) return CUADMM_ERR_INVALID;
  if (fails_out) *fails_out = fails;
  return CUADMM_OK;
}

// ---- the acceleration kernels on host arrays (tests).  State vectors have 2 L entries, the S half right behind the X half: for an
// odd L the S half is then not 16-byte aligned and takes the kernels' one-double path; the engine itself pads (accel.h).
namespace {
struct HookBuf {
  DevBuf<double> d;
  int up(const double* h, size_t n) { int rc = d.alloc(std::max<size_t>(n, 1)); return (rc || !h || !n) ? rc : d.upload(h, n); }
  int down(double* h, size_t n) { return (h && n) ? staged_d2h(h, d.p, sizeof(double) * n) : CUADMM_OK; }
};
}  // namespace
int cuadmm_op_accel_push(int64_t L, const double* u_prev, const double* X, const double* S, double sig, double* f_prev, const double* g_prev, int have_prev,
                         double* g_out, double* dF_out, double* dG_out, double* gnorm2_out) {
  if (L < 1 || !u_prev || !X || !S || !f_prev || !g_out || !gnorm2_out || (have_prev && (!g_prev || !dF_out || !dG_out))) { set_error("op_accel_push: invalid argument"); return CUADMM_ERR_INVALID; }
  int rc = check_device(0);
  if (rc) return rc;
  const size_t n2 = 2 * (size_t)L;
  HookBuf u, x, sv, f, g, dF, dG, part, out;
  if ((rc = u.up(u_prev, n2)) || (rc = x.up(X, L)) || (rc = sv.up(S, L)) || (rc = f.up(f_prev, n2)) || (rc = g.up(have_prev ? g_prev : nullptr, n2)) ||
      (rc = dF.up(dF_out, n2)) || (rc = dG.up(dG_out, n2)) || (rc = part.up(nullptr, kAccelPartials)) || (rc = out.up(nullptr, 1)))
    return rc;
  if ((rc = launch_aa_push(L, L, u.d.p, x.d.p, sv.d.p, sig, f.d.p, g.d.p, have_prev, g.d.p, f.d.p, dF.d.p, dG.d.p, part.d.p, out.d.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipDeviceSynchronize());
  if ((rc = g.down(g_out, n2)) || (rc = f.down(f_prev, n2)) || (rc = dF.down(dF_out, n2)) || (rc = dG.down(dG_out, n2)) || (rc = out.down(gnorm2_out, 1))) return rc;
  return CUADMM_OK;
}
int cuadmm_op_accel_gram(int64_t L2, int cols, int newest, const double* ring_dG, const double* g, double* out) {
  if (L2 < 2 || (L2 & 1) || cols < 1 || cols > kAccelMaxMem || newest < 0 || newest >= cols || !ring_dG || !g || !out) { set_error("op_accel_gram: invalid argument"); return CUADMM_ERR_INVALID; }
  int rc = check_device(0);
  if (rc) return rc;
  HookBuf ring, gv, part, dots;
  if ((rc = ring.up(ring_dG, (size_t)L2 * cols)) || (rc = gv.up(g, L2)) || (rc = part.up(nullptr, kAccelPartials)) || (rc = dots.up(nullptr, kAccelDots))) return rc;
  if ((rc = launch_aa_gram(L2 / 2, L2 / 2, L2, cols, newest, ring.d.p, gv.d.p, part.d.p, dots.d.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipDeviceSynchronize());
  return dots.down(out, 2 * (size_t)cols);
}
int cuadmm_op_accel_combine(int64_t L, int cols, const double* ring_dF, const double* gamma, double sig, double* X_inout, double* S_inout) {
  if (L < 1 || cols < 1 || cols > kAccelMaxMem || !ring_dF || !gamma || !X_inout || !S_inout) { set_error("op_accel_combine: invalid argument"); return CUADMM_ERR_INVALID; }
  int rc = check_device(0);
  if (rc) return rc;
  HookBuf ring, x, sv, u;
  if ((rc = ring.up(ring_dF, 2 * (size_t)L * cols)) || (rc = x.up(X_inout, L)) || (rc = sv.up(S_inout, L)) || (rc = u.up(nullptr, 2 * (size_t)L))) return rc;
  if ((rc = launch_aa_combine(L, L, 2 * L, cols, ring.d.p, gamma, sig, x.d.p, sv.d.p, u.d.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipDeviceSynchronize());
  if ((rc = x.down(X_inout, L)) || (rc = sv.down(S_inout, L))) return rc;
  return CUADMM_OK;
}

// the roll kernel of the infeasibility check on host arrays (csrc/infeas.hip).  offset = 1 places every vector one double behind a
// 16-byte boundary, so that the one-double path runs
int cuadmm_op_infeas_roll(int64_t n, const double* cur, double* prev_inout, const double* w, int negate, int nz, const int64_t* zoff, const int64_t* zlen,
                          int offset, double* d_out, double* sums2_out) {
  if (n < 1 || !cur || !prev_inout || !w || !d_out || !sums2_out || nz < 0 || (nz > 0 && (!zoff || !zlen)) || offset < 0 || offset > 1) {
    set_error("op_infeas_roll: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  for (int r = 0; r < nz; ++r)
    if (zoff[r] < 0 || zlen[r] < 0 || zoff[r] + zlen[r] > n) { set_error("op_infeas_roll: range %d outside the vector", r); return CUADMM_ERR_INVALID; }
  int rc = check_device(0);
  if (rc) return rc;
  const size_t N = (size_t)n + 2;
  DevBuf<double> c, q, wv, out, part, sums;
  DevBuf<long long> zo, zl;
  if ((rc = c.alloc(N)) || (rc = q.alloc(N)) || (rc = wv.alloc(N)) || (rc = out.alloc(N)) || (rc = part.alloc(kInfeasPartials)) || (rc = sums.alloc(2)) ||
      (rc = zo.alloc(std::max(nz, 1))) || (rc = zl.alloc(std::max(nz, 1))))
    return rc;
  if ((rc = staged_h2d(c.p + offset, cur, sizeof(double) * (size_t)n)) || (rc = staged_h2d(q.p + offset, prev_inout, sizeof(double) * (size_t)n)) ||
      (rc = staged_h2d(wv.p + offset, w, sizeof(double) * (size_t)n)))
    return rc;
  if (nz > 0) {
    std::vector<long long> a(zoff, zoff + nz), b(zlen, zlen + nz);
    if ((rc = staged_h2d(zo.p, a.data(), sizeof(long long) * (size_t)nz)) || (rc = staged_h2d(zl.p, b.data(), sizeof(long long) * (size_t)nz))) return rc;
  }
  if ((rc = launch_infeas_roll(n, c.p + offset, q.p + offset, wv.p + offset, out.p + offset, negate, nz, zo.p, zl.p, part.p, sums.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipDeviceSynchronize());
  if ((rc = staged_d2h(prev_inout, q.p + offset, sizeof(double) * (size_t)n)) || (rc = staged_d2h(d_out, out.p + offset, sizeof(double) * (size_t)n)) ||
      (rc = staged_d2h(sums2_out, sums.p, sizeof(double) * 2)))
    return rc;
  return CUADMM_OK;
}

// every block's size and range, before the op hooks of the per-block reductions allocate or launch anything
static int op_check_blocks(const char* who, int64_t n, int nblk, const int* blk, const int64_t* offs) {
  long long o = 0;
  for (int k = 0; k < nblk; ++k) {
    if (blk[k] == 0 || blk[k] > kMaxBlockSize) { set_error("%s: block %d has size %d", who, k, blk[k]); return CUADMM_ERR_INVALID; }
    const long long len = blk_svec_len(blk[k]), off = offs ? (long long)offs[k] : o;
    o += len;
    if (off < 0 || off + len > n) { set_error("%s: block %d outside the vectors", who, k); return CUADMM_ERR_INVALID; }
  }
  return CUADMM_OK;
}

// the per-block norm kernels of the lower bound on host arrays (csrc/lower_bound.hip).  offs: first slot of every block (null: the
// blocks follow one another from slot 0); offset = 1 places both vectors one double behind a 16-byte boundary.  M and P are copied
// back as the kernels left them.
int cuadmm_op_lb_block_norms(int64_t n, double* M_inout, double* P_inout, int nblk, const int* blk, const int64_t* offs, const double* R, int offset,
                             double* pairs_out, double* comb3_out) {
  if (n < 1 || !M_inout || !P_inout || nblk < 1 || !blk || !R || !pairs_out || !comb3_out || offset < 0 || offset > 1) {
    set_error("op_lb_block_norms: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  int rc = op_check_blocks("op_lb_block_norms", n, nblk, blk, offs);
  if (rc || (rc = check_device(0))) return rc;
  cuadmm_solver::BlockTasksDev t;
  const size_t N = (size_t)n + 2;
  DevBuf<double> Md, Pd, Rd, pairs, cpart, out;
  if ((rc = t.build(blk, nblk, offs)) || (rc = Md.alloc(N)) || (rc = Pd.alloc(N)) || (rc = Rd.alloc((size_t)nblk)) || (rc = pairs.alloc(2 * (size_t)nblk)) ||
      (rc = cpart.alloc(2 * (size_t)t.nchunk)) || (rc = out.alloc(4)))
    return rc;
  if ((rc = staged_h2d(Md.p + offset, M_inout, sizeof(double) * (size_t)n)) || (rc = staged_h2d(Pd.p + offset, P_inout, sizeof(double) * (size_t)n)) ||
      (rc = staged_h2d(Rd.p, R, sizeof(double) * (size_t)nblk)))
    return rc;
  CUADMM_HIP_TRY(hipMemset(pairs.p, 0xff, sizeof(double) * pairs.n));
  if ((rc = launch_lb_block_norms(Md.p + offset, Pd.p + offset, t.view(), cpart.p, pairs.p, nullptr))) return rc;
  if ((rc = launch_lb_combine(nblk, pairs.p, Rd.p, t.len.p, t.blk.p, nullptr, out.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipDeviceSynchronize());
  double o4[4];
  if ((rc = staged_d2h(M_inout, Md.p + offset, sizeof(double) * (size_t)n)) || (rc = staged_d2h(P_inout, Pd.p + offset, sizeof(double) * (size_t)n)) ||
      (rc = staged_d2h(pairs_out, pairs.p, sizeof(double) * 2 * (size_t)nblk)) || (rc = staged_d2h(o4, out.p, sizeof(double) * 4)))
    return rc;
  comb3_out[0] = o4[0]; comb3_out[1] = o4[1]; comb3_out[2] = o4[2];
  return CUADMM_OK;
}

// the per-block statistics kernels of cuadmm_evaluate on host arrays (csrc/evaluate.hip).  offs and offset as in cuadmm_op_lb_block_norms;
// every block's size and range is validated before anything is launched.  The five vectors are copied back as the kernels left them.
int cuadmm_op_ev_block_stats(int64_t n, double* X, double* S, double* PX, double* PS, double* Rd1, int nblk, const int* blk, const int64_t* offs, int offset,
                             double* sums6_out) {
  if (n < 1 || !X || !S || !PX || !PS || !Rd1 || nblk < 1 || !blk || !sums6_out || offset < 0 || offset > 1) {
    set_error("op_ev_block_stats: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  int rc = op_check_blocks("op_ev_block_stats", n, nblk, blk, offs);
  if (rc || (rc = check_device(0))) return rc;
  cuadmm_solver::BlockTasksDev t;
  const size_t N = (size_t)n + 2;
  double* const host[5] = {X, S, PX, PS, Rd1};
  DevBuf<double> v[5], sums, cpart;
  for (int q = 0; q < 5; ++q)
    if ((rc = v[q].alloc(N)) || (rc = staged_h2d(v[q].p + offset, host[q], sizeof(double) * (size_t)n))) return rc;
  if ((rc = t.build(blk, nblk, offs)) || (rc = sums.alloc(kEvSums * (size_t)nblk)) || (rc = cpart.alloc(kEvSums * (size_t)t.nchunk))) return rc;
  CUADMM_HIP_TRY(hipMemset(sums.p, 0xff, sizeof(double) * sums.n));
  if ((rc = launch_ev_block_stats(v[0].p + offset, v[1].p + offset, v[2].p + offset, v[3].p + offset, v[4].p + offset, t.view(), cpart.p, sums.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipDeviceSynchronize());
  for (int q = 0; q < 5; ++q)
    if ((rc = staged_d2h(host[q], v[q].p + offset, sizeof(double) * (size_t)n))) return rc;
  return staged_d2h(sums6_out, sums.p, sizeof(double) * kEvSums * (size_t)nblk);
}

// the lambda_min kernel on a device vector whose blocks follow one another from slot 0 (csrc/lambda_min.hip); blk_vals on the host
int cuadmm_op_block_lambda_min(const double* svec_dev, const int* blk_vals, int mat_num, int steps, double* per_block3_host, void* stream) {
  if (!svec_dev || !blk_vals || mat_num < 1 || !per_block3_host || steps < 1 || steps > kLmStepsMax) { set_error("op_block_lambda_min: invalid argument"); return CUADMM_ERR_INVALID; }
  for (int k = 0; k < mat_num; ++k)
    if (blk_vals[k] == 0 || blk_vals[k] > kMaxBlockSize) { set_error("op_block_lambda_min: block %d has size %d", k, blk_vals[k]); return CUADMM_ERR_INVALID; }
  int rc, ndev = 0;      // the current device is the vector's: it is not changed
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this engine has no CPU fallback"); return CUADMM_ERR_NO_DEVICE; }
  hipStream_t st = (hipStream_t)stream;
  cuadmm_solver::BlockTasksDev t;
  cuadmm_solver::LmPlan plan;
  if ((rc = t.build(blk_vals, mat_num, nullptr)) || (rc = plan.build(blk_vals, mat_num))) return rc;
  if ((rc = plan.run(svec_dev, 1.0, t.off.p, t.blk.p, steps, st))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  std::vector<double> h(kLmOut * (size_t)mat_num);
  if ((rc = staged_d2h(h.data(), plan.out.p, sizeof(double) * h.size()))) return rc;
  for (int k = 0; k < mat_num; ++k)
    for (int q = 0; q < 3; ++q) per_block3_host[3 * k + q] = h[kLmOut * (size_t)k + q];
  return CUADMM_OK;
}

// the lowrank kernel on a device vector whose blocks follow one another from slot 0 (csrc/lowrank.hip); blk_vals on the host
int cuadmm_op_block_lowrank(const double* svec_dev, const int* blk_vals, int mat_num, double tol, int rmax, double* per_block6_host, double* L_host, int* piv_host,
                            void* stream) {
  if (!svec_dev || !blk_vals || mat_num < 1 || !per_block6_host || !(tol >= 0.0 && tol < 1.0) || rmax < 1 || rmax > kMaxBlockSize) {
    set_error("op_block_lowrank: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  for (int k = 0; k < mat_num; ++k)
    if (blk_vals[k] == 0 || blk_vals[k] > kMaxBlockSize) { set_error("op_block_lowrank: block %d has size %d", k, blk_vals[k]); return CUADMM_ERR_INVALID; }
  int rc, ndev = 0;      // the current device is the vector's: it is not changed
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this engine has no CPU fallback"); return CUADMM_ERR_NO_DEVICE; }
  hipStream_t st = (hipStream_t)stream;
  cuadmm_solver::BlockTasksDev t;
  cuadmm_solver::LrPlan plan;
  if ((rc = t.build(blk_vals, mat_num, nullptr)) || (rc = plan.prepare(blk_vals, mat_num, rmax))) return rc;
  if ((rc = plan.run(svec_dev, 1.0, t.off.p, t.blk.p, tol, st))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  return plan.fetch(1.0, per_block6_host, L_host, piv_host);
}

int cuadmm_dev_malloc(void** ptr, size_t bytes) { CUADMM_HIP_TRY(hipMalloc(ptr, bytes ? bytes : 8)); return CUADMM_OK; }
int cuadmm_dev_free(void* ptr) { if (ptr) CUADMM_HIP_TRY(hipFree(ptr)); return CUADMM_OK; }
int cuadmm_memcpy_h2d(void* dst, const void* src, size_t bytes) { return staged_h2d(dst, src, bytes); }
int cuadmm_memcpy_d2h(void* dst, const void* src, size_t bytes) { return staged_d2h(dst, src, bytes); }
int cuadmm_dev_sync(void) { CUADMM_HIP_TRY(hipDeviceSynchronize()); return CUADMM_OK; }

// ------------------------------------------------------------------------------------------
// TXT problem objects
// ------------------------------------------------------------------------------------------
struct cuadmm_problem { ProblemData d; };

int cuadmm_problem_from_txt(const char* prefix, cuadmm_problem** out) {
  if (!prefix || !out) { set_error("problem_from_txt: null"); return CUADMM_ERR_INVALID; }
  cuadmm_problem* p = new cuadmm_problem();
  int rc = load_problem_txt(prefix, p->d, true);
  if (rc) { delete p; return rc; }
  *out = p;
  return CUADMM_OK;
}
int cuadmm_problem_view_get(const cuadmm_problem* p, cuadmm_problem_view* v) {
  if (!p || !v) { set_error("problem_view: null"); return CUADMM_ERR_INVALID; }
  const ProblemData& d = p->d;
  v->vec_len = d.vec_len; v->con_num = d.con_num; v->mat_num = d.mat_num;
  v->At_nnz = (int)d.At_vals.size(); v->b_nnz = (int)d.b_vals.size(); v->C_nnz = (int)d.C_vals.size();
  v->At_csc_col_ptrs = d.At_col_ptrs.data(); v->At_csc_row_ids = d.At_row_ids.data(); v->At_csc_vals = d.At_vals.data();
  v->b_indices = d.b_idx.data(); v->b_vals = d.b_vals.data(); v->C_indices = d.C_idx.data(); v->C_vals = d.C_vals.data();
  v->blk_vals = d.blk.data();
  return CUADMM_OK;
}
void cuadmm_problem_free(cuadmm_problem* p) { delete p; }

int cuadmm_coo_to_csc(int* col_ptrs, int* col_ids, int* row_ids, double* vals, int nnz, int col_num) {
  if (nnz < 0 || col_num < 0 || !col_ptrs) { set_error("coo_to_csc: bad arguments"); return CUADMM_ERR_INVALID; }
  std::vector<int> cp, c(col_ids, col_ids + nnz), r(row_ids, row_ids + nnz);
  std::vector<double> v(vals, vals + nnz);
  coo_to_csc(cp, c, r, v, nnz, col_num);
  std::copy(cp.begin(), cp.end(), col_ptrs);
  std::copy(c.begin(), c.end(), col_ids);
  std::copy(r.begin(), r.end(), row_ids);
  std::copy(v.begin(), v.end(), vals);
  return CUADMM_OK;
}

int cuadmm_read_blk(const char* filename, char* types, int* sizes, int cap) {
  std::vector<char> t;
  std::vector<int> sz;
  int rc = read_blk_file(filename, t, sz);
  if (rc) return rc;
  for (size_t i = 0; i < sz.size() && (int)i < cap; ++i) { if (types) types[i] = t[i]; if (sizes) sizes[i] = sz[i]; }
  return (int)sz.size();
}

int cuadmm_read_sparse_vec_txt(const char* filename, int* indices, double* vals, int cap) {
  if (!filename) { set_error("read_sparse_vec_txt: null"); return CUADMM_ERR_INVALID; }
  std::vector<int> idx, zero;
  std::vector<double> v;
  int rc = read_triplets(filename, idx, zero, v, false);
  if (rc) return rc;
  for (size_t i = 0; i < v.size() && (int)i < cap; ++i) { if (indices) indices[i] = idx[i]; if (vals) vals[i] = v[i]; }
  return (int)v.size();
}

int cuadmm_write_dense_txt(const char* filename, const double* vals, int64_t n) {
  FILE* f = fopen(filename, "w");
  if (!f) { set_error("Failed to open file: %s", filename); return CUADMM_ERR_IO; }
  for (int64_t i = 0; i < n; ++i) fprintf(f, "%.32f\n", vals[i]);     // memory.h:278-294
  fclose(f);
  return CUADMM_OK;
}

}  // extern "C"
