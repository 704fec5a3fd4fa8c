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

#include "engine_state.h"

using namespace cuadmm;

namespace cuadmm {
RcclApi g_rccl;
}  // namespace cuadmm

int cuadmm::check_device(int device) {
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
namespace cuadmm {

// max(1, ||v[lo, hi)||): what a constraint's column is divided by (get_normA, sparse_matrix_norm.cu:11-31)
double cons_norm(const double* v, int lo, int hi) {
  double nrm = 0.0;
  for (int p = lo; p < hi; ++p) nrm += v[p] * v[p];
  return std::max(1.0, std::sqrt(nrm));
}

double sum_sq(const double* v, int n) {
  double t = 0;
  for (int i = 0; i < n; ++i) t += v[i] * v[i];
  return t;
}
// the indices of a sparse vector (`what` of entry point `who`): inside [0, n), none twice (the norms would count both entries, the vector one)
int check_sparse_idx(const char* who, const char* what, const int* idx, int nnz, long long n) {
  std::vector<char> seen((size_t)n, 0);
  for (int i = 0; i < nnz; ++i) {
    if (idx[i] < 0 || idx[i] >= n) { set_error("%s: %s index %d out of range", who, what, idx[i]); return CUADMM_ERR_INVALID; }
    if (seen[idx[i]]) { set_error("%s: %s index %d appears twice", who, what, idx[i]); return CUADMM_ERR_INVALID; }
    seen[idx[i]] = 1;
  }
  return CUADMM_OK;
}
// sum (val_i / norm[idx_i])^2 over the entries, in their order (sparse_dense.cu:11-20)
double sum_scaled_sq(const int* idx, const double* val, int nnz, const double* norm) {
  double t = 0;
  for (int i = 0; i < nnz; ++i) { const double v = val[i] / norm[idx[i]]; t += v * v; }
  return t;
}
// full[j] = val_i / normA[j] for the entries of this rank (j = g2l[idx_i], -1: another rank's; g2l null: j = idx_i); returns their sum of squares
double scaled_b(const int* idx, const double* val, int nnz, const int* g2l, const std::vector<double>& normA, std::vector<double>& full) {
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
      for (int j = 0; j < 2; ++j) if ((rc = s->ev0[k][j].create()) || (rc = s->ev1[k][j].create())) return rc;

  s->m = m; s->L_full = vec_len; s->nblk_full = mat_num; s->sig = sig;

  return rc;
}

// stage: get_normA and A^T in CSR over the svec rows (what the factor and the device matrices are built from)
int init_normalise(Solver* s, const InitIn& in, InitCtx& c) {
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
int tail_probe(Solver* s, const int64_t* srp, const int* sci, const double* sv, int tk, bool& tail_ok) {
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
int init_solve_plan(Solver* s, const InitIn& in, InitCtx& c) {
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
int init_closed(Solver* s, const InitIn& in, InitCtx& c) {
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
int init_residuals(Solver* s, bool y_resident) {
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
}  // namespace cuadmm

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

static_assert(kOptAccelMaxMem == kAccelMaxMem, "option_table.h: the bound of accel");
// lookup -> check -> normalise -> store -> log -> forward: what a key takes and where it goes are the rows of the two tables (option_table.h,
// psd_options.h); a refused value leaves the solver and its log as they were
int cuadmm_set_option(cuadmm_solver* s, const char* key, double value) {
  if (!s || !key) { set_error("set_option: null"); return CUADMM_ERR_INVALID; }
  const OptionSpec<cuadmm_solver>* eng = engine_option_table<cuadmm_solver>().find(key);
  const OptionSpec<PsdOptions>* psd = eng ? nullptr : psd_option_table().find(key);
  const OptionRow* row = eng ? static_cast<const OptionRow*>(eng) : psd;
  if (!row) { set_error("set_option: unknown key '%s'", key); return CUADMM_ERR_INVALID; }
  double v = 0;
  switch (option_check(*row, value, &v)) {
    case kOptInvalid: set_error("%s", row->refusal); return CUADMM_ERR_INVALID;
    case kOptNotFinite: set_error("set_option: %s takes a finite value", key); return CUADMM_ERR_INVALID;
    case kOptOutOfRange: set_error("set_option: %s is out of range", key); return CUADMM_ERR_INVALID;
    case kOptOk: break;
  }
  if (row->when == kBeforeInit && s->initialised) { set_error("set_option: %s is set before init", key); return CUADMM_ERR_INVALID; }
  if (eng) eng->field(*s, &v);
  else psd->field(s->plan.opt, &v);
  if (row->group == kGroupInject && s->group) duo_group_inject(s->group, s->duo_inject);
  if (row->group != kGroupPerRank) s->option_log.emplace_back(key, value);      // the log is what a group replays on its new ranks
  // a group handle: every rank follows -- AFTER the key has been validated on the leader; a child that refuses leaves the option
  // out of the log (it is not replayed on later children) and the error with the caller
  if (s->group && !s->in_group_call && row->group == kGroupShared)
    for (int r = 1; r < duo_group_world(s->group); ++r) {
      int rc = cuadmm_set_option(duo_group_rank(s->group, r), key, value);
      if (rc) { s->option_log.pop_back(); return rc; }
    }
  return CUADMM_OK;
}

// read-only views of the two tables, the engine's rows first (host only; nothing in the engine calls them)
int cuadmm_option_count(void) { return engine_option_table<cuadmm_solver>().n + psd_option_table().n; }
int cuadmm_option_info(int i, const char** key, const char** env, double* def, unsigned* flags) {
  const int ne = engine_option_table<cuadmm_solver>().n;
  if (i < 0 || i >= cuadmm_option_count()) { set_error("option_info: no option %d", i); return CUADMM_ERR_INVALID; }
  const OptionRow& o = i < ne ? static_cast<const OptionRow&>(engine_option_table<cuadmm_solver>().rows[i]) : psd_option_table().rows[i - ne];
  if (key) *key = o.key;
  if (env) *env = o.env;
  if (def) *def = o.def;
  if (flags) *flags = o.flags() | (i < ne ? 0u : 256u);
  return CUADMM_OK;
}
int cuadmm_get_option(cuadmm_solver* s, const char* key, double* value) {
  if (!s || !key || !value) { set_error("get_option: null"); return CUADMM_ERR_INVALID; }
  if (const OptionSpec<cuadmm_solver>* o = engine_option_table<cuadmm_solver>().find(key)) *value = option_get(*o, *s);
  else if (const OptionSpec<PsdOptions>* p = psd_option_table().find(key)) *value = option_get(*p, s->plan.opt);
  else { set_error("get_option: unknown key '%s'", key); return CUADMM_ERR_INVALID; }
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
  const struct { bool on; const char* option; const char* why; } single_engine[] = {
      {s->aa.mem > 0, "accel", "Gram matrix is"}, {s->inf.period > 0, "infeas_check", "sums are"}, {s->lb.period > 0, "gap_check", "sums are"}};
  for (const auto& f : single_engine)
    if (device_num_requested > 1 && f.on) {
      set_error("duo_init: option %s works on one engine (device_num_requested = %d): its %s not all-reduced", f.option, device_num_requested, f.why);
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
}  // extern "C"
