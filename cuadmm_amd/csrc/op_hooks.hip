// Op-level entry points (cuadmm_op_*, cuadmm_psd_plan_*): single kernels and plans on the caller's arrays, for tests and tools, and the C
// wrappers of the TXT problem loader.  No solver handle is touched here.  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "dev_buf.h"
#include "report_plans.h"
#include "tail_solve.h"
#include "lead_solve.h"
#include "vec_kernels.h"
#include "accel.h"
#include "infeas.h"
#include "lower_bound.h"
#include "evaluate.h"

using namespace cuadmm;

extern "C" {

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

// one pair of a test hook's options; a known key with a value no key takes (not finite, beyond an int) is not called unknown
static int psd_option_from_pair(const char* who, const char* key, double value, PsdOptions& opt) {
  OptCheck why = kOptOk;
  if (key && opt.set(key, value, &why)) return CUADMM_OK;
  if (!key || why == kOptOk) set_error("%s: unknown option %s", who, key ? key : "(null)");
  else set_error(why == kOptNotFinite ? "%s: option %s takes a finite value" : "%s: option %s is out of range", who, key);
  return CUADMM_ERR_INVALID;
}
// the default options (NOT the environment's) changed by opt_keys[n_opts] = opt_vals[n_opts]
static int psd_options_from_pairs(const char* who, const char* const* opt_keys, const double* opt_vals, int n_opts, PsdOptions& opt) {
  if (n_opts < 0 || (n_opts > 0 && (!opt_keys || !opt_vals))) { set_error("%s: bad arguments", who); return CUADMM_ERR_INVALID; }
  opt = PsdOptions();
  for (int i = 0; i < n_opts; ++i)
    if (int rc = psd_option_from_pair(who, opt_keys[i], opt_vals[i], opt)) return rc;
  return CUADMM_OK;
}

// cuadmm_op_psd_project_ex on a plan whose options are PsdOptions() changed by the pairs given: no environment variable reaches it, so a
// test runs the variant it names
int cuadmm_op_psd_project_opts(const double* Xb, double* Xproj, const int* blk_host, int mat_num, int eig_rank, const char* const* opt_keys,
                               const double* opt_vals, int n_opts, int* steps_dev, void* stream) {
  if (!blk_host || mat_num < 0 || eig_rank < 0) { set_error("psd_project_opts: bad arguments"); return CUADMM_ERR_INVALID; }
  PsdPlan plan;
  int rc = psd_options_from_pairs("psd_project_opts", opt_keys, opt_vals, n_opts, plan.opt);
  if (rc) return rc;
  plan.eig_rank = eig_rank;
  if ((rc = plan.build(blk_host, mat_num))) return rc;
  if (steps_dev) {
    CUADMM_HIP_TRY(hipMemsetAsync(steps_dev, 0, sizeof(int) * (size_t)mat_num, (hipStream_t)stream));
    plan.d_steps = steps_dev;
    plan.sign.d_steps = steps_dev;
  }
  if ((rc = plan.project(Xb, Xproj, (hipStream_t)stream))) return rc;
  int fails = plan.fail_count((hipStream_t)stream);   // synchronises the stream
  if (fails != 0) { set_error("psd_project_opts: %d blocks hit the QL sweep cap", fails); return CUADMM_ERR_EIG; }
  return CUADMM_OK;
}

// host only: the sign path's groups of these blocks, merged ones first (they share the first launch), then the others in the order they run
int cuadmm_psd_sign_groups(const int* blk_host, int mat_num, const char* const* opt_keys, const double* opt_vals, int n_opts, int* out, int cap,
                           int* n_groups_out) {
  if (!blk_host || mat_num < 0 || !out || cap < 0 || !n_groups_out) { set_error("psd_sign_groups: bad arguments"); return CUADMM_ERR_INVALID; }
  PsdPlan plan;
  int rc = psd_options_from_pairs("psd_sign_groups", opt_keys, opt_vals, n_opts, plan.opt);
  if (rc || (rc = plan.build_host(blk_host, mat_num))) return rc;
  std::vector<int> members, ids;
  for (int k = 0; k < mat_num; ++k)
    if (blk_host[k] >= plan.ranges.sign_min) members.push_back(k);
  SignPsd::Sizes sz;
  plan.sign.opt = plan.opt;
  plan.sign.build_host(blk_host, members, ids, sz);
  *n_groups_out = (int)plan.sign.groups.size();
  if (*n_groups_out > cap) { set_error("psd_sign_groups: %d groups, room for %d", *n_groups_out, cap); return CUADMM_ERR_INVALID; }
  for (int merged = 1; merged >= 0; --merged)
    for (const SignPsd::Group& g : plan.sign.groups)
      if ((int)g.merged == merged) { plan.sign.group_info(g, out); out += SignPsd::kGroupInfo; }
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
    if (int rc = psd_option_from_pair("psd_plan_ranges", opt_keys[i], opt_vals[i], plan.opt)) return rc;
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
  BlockTasksDev t;
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
  BlockTasksDev t;
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
  BlockTasksDev t;
  LmPlan plan;
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
  BlockTasksDev t;
  LrPlan plan;
  if ((rc = t.build(blk_vals, mat_num, nullptr)) || (rc = plan.prepare(blk_vals, mat_num, rmax))) return rc;
  if ((rc = plan.run(svec_dev, 1.0, t.off.p, t.blk.p, tol, st))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  return plan.fetch(1.0, per_block6_host, L_host, piv_host);
}

// What the three factor hooks below refuse block by block, in their own wording: a size the plans do not take, a rank outside
// 0 .. factor_cols, a positive rank while a buffer is missing (have = false; null_text says which).
static int op_check_ranks(const char* who, const int* blk_vals, int mat_num, const int* ranks, int rmax, bool have, const char* null_text) {
  for (int k = 0; k < mat_num; ++k) {
    const int n = blk_vals[k];
    if (n == 0 || n > kMaxBlockSize) { set_error("%s: block %d has size %d", who, k, n); return CUADMM_ERR_INVALID; }
    if (n > 0 && (ranks[k] < 0 || ranks[k] > factor_cols(n, rmax) || (ranks[k] > 0 && !have))) {
      set_error("%s: block %d of size %d has rank %d%s", who, k, n, ranks[k], have ? "" : null_text);
      return CUADMM_ERR_INVALID;
    }
  }
  return CUADMM_OK;
}

// the kernel of cuadmm_set_lowrank on a DEVICE svec vector whose blocks follow one another from slot 0 (csrc/lowrank_apply.hip); the factor
// buffer (csrc/factor_layout.h, for rmax), ranks and blk_vals on the host.  Synchronises the stream.
int cuadmm_op_block_outer(const double* L_host, const int* ranks, const int* blk_vals, int mat_num, int rmax, double* svec_dev_inout, void* stream) {
  if (!ranks || !blk_vals || mat_num < 1 || rmax < 1 || rmax > kMaxBlockSize || !svec_dev_inout) { set_error("op_block_outer: invalid argument"); return CUADMM_ERR_INVALID; }
  int rc = op_check_ranks("op_block_outer", blk_vals, mat_num, ranks, rmax, L_host != nullptr, " and L is null"), ndev = 0;
  if (rc) return rc;      // the current device is the vector's: it is not changed
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this engine has no CPU fallback"); return CUADMM_ERR_NO_DEVICE; }
  hipStream_t st = (hipStream_t)stream;
  BlockTasksDev t;
  FactorLayoutDev fl;
  LoPlan plan;
  if ((rc = t.build(blk_vals, mat_num, nullptr)) || (rc = fl.prepare(blk_vals, mat_num, rmax)) || (rc = plan.prepare(fl, blk_vals)) ||
      (rc = fl.stage(plan.Lbuf, L_host)) || (rc = fl.stage_ranks(ranks)))
    return rc;
  if ((rc = plan.run(fl, plan.Lbuf.p, t.off.p, t.blk.p, svec_dev_inout, st))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  return CUADMM_OK;
}

// the host side of that kernel: loff_out (mat_num + 1, may be null) <- the factor offsets for rmax; tasks_out (may be null) <- up to
// cap_slots wavefront slots of four ints (k, t0, t1, step).  split_from: the size from which a block is split over workgroups (0: the
// engine's).  Returns the number of slots.  Host only.
int cuadmm_op_block_outer_plan(const int* blk_vals, int mat_num, int rmax, int split_from, long long* loff_out, int* tasks_out, int cap_slots) {
  std::vector<LoTask> tasks;
  std::vector<long long> loff;
  int rc = lo_build_tasks(mat_num, blk_vals, rmax, split_from ? split_from : kLoSplitFrom, &tasks, &loff);
  if (rc) return rc;
  if (loff_out) std::copy(loff.begin(), loff.end(), loff_out);
  for (size_t q = 0; tasks_out && q < tasks.size() && (int)q < cap_slots; ++q) {
    tasks_out[4 * q] = tasks[q].k; tasks_out[4 * q + 1] = tasks[q].t0; tasks_out[4 * q + 2] = tasks[q].t1; tasks_out[4 * q + 3] = tasks[q].step;
  }
  return (int)tasks.size();
}

// the kernel of cuadmm_block_multiply on a DEVICE svec vector whose blocks follow one another from slot 0 (csrc/block_mult.hip): W_host <-
// sign * M_k V_k per PSD block, + 0.0 in the columns >= ranks[k]; V_host (null where every rank is 0) and W_host laid out as
// cuadmm_lowrank's L_out for rmax, ranks and blk_vals on the host.  The vector is only read.  Synchronises the stream.
int cuadmm_op_block_mult(const double* svec_dev, const int* blk_vals, int mat_num, double sign, const double* V_host, const int* ranks, int rmax, double* W_host,
                         void* stream) {
  if (!svec_dev || !ranks || !blk_vals || mat_num < 1 || rmax < 1 || rmax > kMaxBlockSize || !W_host || !(sign == 1.0 || sign == -1.0)) {
    set_error("op_block_mult: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  int rc = op_check_ranks("op_block_mult", blk_vals, mat_num, ranks, rmax, V_host != nullptr, " and V is null"), ndev = 0;
  if (rc) return rc;      // the current device is the vector's: it is not changed
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this engine has no CPU fallback"); return CUADMM_ERR_NO_DEVICE; }
  hipStream_t st = (hipStream_t)stream;
  BlockTasksDev t;
  FactorLayoutDev fl;
  BmPlan plan;
  if ((rc = t.build(blk_vals, mat_num, nullptr)) || (rc = fl.prepare(blk_vals, mat_num, rmax)) || (rc = plan.prepare(fl, blk_vals)) ||
      (rc = fl.stage(plan.Vbuf, V_host)) || (rc = fl.stage_ranks(ranks)))
    return rc;
  if ((rc = plan.run(fl, svec_dev, sign, t.off.p, t.blk.p, st))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  return plan.fetch(fl, blk_vals, ranks, 1.0, W_host);
}

// the host side of that kernel: loff_out (mat_num + 1, may be null) <- the offsets of V_k / W_k for rmax; tasks_out (may be null) <- up to
// cap_slots wavefront slots of two ints (k, panel; k < 0: an empty slot).  Returns the number of slots.  Host only.
int cuadmm_op_block_mult_plan(const int* blk_vals, int mat_num, int rmax, long long* loff_out, int* tasks_out, int cap_slots) {
  std::vector<BmTask> tasks;
  std::vector<long long> loff;
  int rc = bm_build_tasks(mat_num, blk_vals, rmax, &tasks, &loff);
  if (rc) return rc;
  if (loff_out) std::copy(loff.begin(), loff.end(), loff_out);
  for (size_t q = 0; tasks_out && q < tasks.size() && (int)q < cap_slots; ++q) { tasks_out[2 * q] = tasks[q].k; tasks_out[2 * q + 1] = tasks[q].p; }
  return (int)tasks.size();
}

// the multiplier pass of cuadmm_lowrank_grad on host arrays of m doubles in the engine's scaled space (csrc/lowrank_grad.h, xunit = 1):
// ytilde_out <- the scaled y - sigma r, r_out <- r in the caller's units, out2 <- [y'r in the caller's units, ||r||^2] from the kernel's
// slot partials added in slot order.  The default stream, synchronised.
int cuadmm_op_lrg_multiplier(int m, const double* ax, const double* b, const double* normA, const double* y, double bscale, double Cscale, double sigma,
                             double* ytilde_out, double* r_out, double out2[2]) {
  if (m < 1 || !ax || !b || !normA || !y || !ytilde_out || !r_out || !out2 || !(sigma >= 0.0) || !std::isfinite(sigma) || !(bscale > 0) || !(Cscale > 0)) {
    set_error("op_lrg_multiplier: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  int rc, ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this engine has no CPU fallback"); return CUADMM_ERR_NO_DEVICE; }
  DevBuf<double> in[4], yt, r, part;
  const double* const src[4] = {ax, b, normA, y};
  for (int q = 0; q < 4; ++q)
    if ((rc = in[q].alloc((size_t)m)) || (rc = in[q].upload(src[q], (size_t)m))) return rc;
  if ((rc = yt.alloc((size_t)m)) || (rc = r.alloc((size_t)m)) || (rc = part.alloc(2 * (size_t)kBrSlots))) return rc;
  if ((rc = launch_lrg_multiplier(m, in[0].p, in[1].p, in[2].p, in[3].p, 1.0, bscale, 1 / Cscale, sigma, yt.p, r.p, part.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  std::vector<double> h(2 * (size_t)kBrSlots);
  if ((rc = staged_d2h(ytilde_out, yt.p, sizeof(double) * (size_t)m)) || (rc = staged_d2h(r_out, r.p, sizeof(double) * (size_t)m)) ||
      (rc = staged_d2h(h.data(), part.p, sizeof(double) * h.size())))
    return rc;
  out2[0] = slot_sum(h.data()) * (bscale * Cscale);
  out2[1] = slot_sum(h.data() + kBrSlots);
  return CUADMM_OK;
}

// the outer-product kernel of cuadmm_lowrank_line on three DEVICE svec vectors whose blocks follow one another from slot 0
// (csrc/lowrank_line.hip); the factor buffers (one layout), ranks and blk_vals on the host.  The task list is LoPlan's, that of
// cuadmm_op_block_outer_plan(split_from).  Synchronises the stream.
int cuadmm_op_block_outer3(const double* L_host, const double* D_host, const int* ranks, const int* blk_vals, int mat_num, int rmax, int split_from,
                           double* x0_dev_inout, double* x1_dev_inout, double* x2_dev_inout, void* stream) {
  if (!ranks || !blk_vals || mat_num < 1 || rmax < 1 || rmax > kMaxBlockSize || !x0_dev_inout || !x1_dev_inout || !x2_dev_inout) {
    set_error("op_block_outer3: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  int rc = op_check_ranks("op_block_outer3", blk_vals, mat_num, ranks, rmax, L_host && D_host, " and L or D is null"), ndev = 0;
  if (rc) return rc;
  std::vector<LoTask> probe;             // the planner's own refusals (split_from) before any device work
  if ((rc = lo_build_tasks(mat_num, blk_vals, rmax, split_from ? split_from : kLoSplitFrom, &probe, nullptr))) return rc;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this engine has no CPU fallback"); return CUADMM_ERR_NO_DEVICE; }
  hipStream_t st = (hipStream_t)stream;  // the current device is the vectors': it is not changed
  BlockTasksDev t;
  FactorLayoutDev fl;
  LoPlan plan;
  DevBuf<double> Dbuf;
  const bool both = L_host && D_host;
  if ((rc = t.build(blk_vals, mat_num, nullptr)) || (rc = fl.prepare(blk_vals, mat_num, rmax)) ||
      (rc = plan.prepare(fl, blk_vals, split_from ? split_from : kLoSplitFrom)) || (rc = Dbuf.alloc(fl.count() + 1)) ||
      (rc = fl.stage(plan.Lbuf, both ? L_host : nullptr)) || (rc = fl.stage(Dbuf, both ? D_host : nullptr)) || (rc = fl.stage_ranks(ranks)))
    return rc;
  if ((rc = launch_block_outer3((int)plan.tasks.size(), plan.tasks_d.p, plan.Lbuf.p, Dbuf.p, fl.loff_d.p, fl.ranks_d.p, t.off.p, t.blk.p, x0_dev_inout,
                                x1_dev_inout, x2_dev_inout, st)))
    return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  return CUADMM_OK;
}

// the streaming pass of cuadmm_lowrank_line on host arrays of m doubles in the engine's scaled space (csrc/lowrank_line.h, xunit = 1).
// Each device vector starts in the 16-byte phase of its host array, so that a caller's view chooses the element-to-thread map.  out9 from
// the kernel's slot partials added in slot order, the first three times bscale Cscale.  The default stream, synchronised.
int cuadmm_op_lrl_sums(int m, const double* ax0, const double* ax1, const double* ax2, const double* b, const double* normA, const double* y, double bscale,
                       double Cscale, double* r_out, double* p_out, double* q_out, double out9[9]) {
  if (m < 1 || !ax0 || !ax1 || !ax2 || !b || !normA || !y || !r_out || !p_out || !q_out || !out9 || !(bscale > 0) || !(Cscale > 0)) {
    set_error("op_lrl_sums: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  int rc, ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this engine has no CPU fallback"); return CUADMM_ERR_NO_DEVICE; }
  DevBuf<double> buf[9], part;
  double* dev[9];
  const double* const src[9] = {ax0, ax1, ax2, b, normA, y, r_out, p_out, q_out};
  for (int v = 0; v < 9; ++v) {
    if ((rc = buf[v].alloc((size_t)m + 2))) return rc;
    dev[v] = buf[v].p + ((reinterpret_cast<uintptr_t>(src[v]) >> 3) & 1);
    if (v < 6 && (rc = staged_h2d(dev[v], src[v], sizeof(double) * (size_t)m))) return rc;
  }
  if ((rc = part.alloc(kLlParts * (size_t)kBrSlots))) return rc;
  if ((rc = launch_lrl_sums(m, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], 1.0, bscale, dev[6], dev[7], dev[8], part.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  std::vector<double> h(kLlParts * (size_t)kBrSlots);
  if ((rc = staged_d2h(r_out, dev[6], sizeof(double) * (size_t)m)) || (rc = staged_d2h(p_out, dev[7], sizeof(double) * (size_t)m)) ||
      (rc = staged_d2h(q_out, dev[8], sizeof(double) * (size_t)m)) || (rc = staged_d2h(h.data(), part.p, sizeof(double) * h.size())))
    return rc;
  for (int j = 0; j < kLlParts; ++j) {
    const double sum = slot_sum(h.data() + (size_t)j * kBrSlots);
    out9[j] = j < 3 ? sum * (bscale * Cscale) : sum;
  }
  return CUADMM_OK;
}

// The three streaming kernels of cuadmm_lowrank_refine on host arrays (csrc/lowrank_refine.h).  Each device vector starts in the 16-byte
// phase of its host array, so that a caller's view chooses the element-to-thread map.  An array a kernel writes has n + 1 doubles: entry n
// is a guard that travels to the device and back and must come back with its bits.  The default stream, synchronised.
static int lrr_stage(int nv, const double* const* src, const long long* len, DevBuf<double>* buf, double** dev) {
  int rc;
  for (int v = 0; v < nv; ++v) {
    if ((rc = buf[v].alloc((size_t)len[v] + 2))) return rc;
    dev[v] = buf[v].p + ((reinterpret_cast<uintptr_t>(src[v]) >> 3) & 1);
    if ((rc = staged_h2d(dev[v], src[v], sizeof(double) * (size_t)len[v]))) return rc;
  }
  return CUADMM_OK;
}
static int lrr_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available; this engine has no CPU fallback"); return CUADMM_ERR_NO_DEVICE; }
  return CUADMM_OK;
}
// out3 <- gg, go, gd of G = 2 (unit W): the kernel's slot partials added in slot order
int cuadmm_op_lrr_dots(long long n, const double* W, double unit, const double* G_old, const double* D_old, double out3[3]) {
  if (n < 1 || !W || !G_old || !D_old || !out3) { set_error("op_lrr_dots: invalid argument"); return CUADMM_ERR_INVALID; }
  int rc = lrr_device();
  if (rc) return rc;
  DevBuf<double> buf[3], part;
  double* dev[3];
  const double* const src[3] = {W, G_old, D_old};
  const long long len[3] = {n, n, n};
  if ((rc = lrr_stage(3, src, len, buf, dev)) || (rc = part.alloc(kRfParts * (size_t)kBrSlots))) return rc;
  if ((rc = launch_lrr_dots(n, dev[0], unit, dev[1], dev[2], part.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  std::vector<double> h(kRfParts * (size_t)kBrSlots);
  if ((rc = staged_d2h(h.data(), part.p, sizeof(double) * h.size()))) return rc;
  for (int j = 0; j < kRfParts; ++j) out3[j] = slot_sum(h.data() + (size_t)j * kBrSlots);
  return CUADMM_OK;
}
// D_inout, Ds_out, Gold_out: n + 1 doubles each (the guard last); W: n
int cuadmm_op_lrr_direction(long long n, const double* W, double unit, double beta, int restart, double root, double* D_inout, double* Ds_out, double* Gold_out) {
  if (n < 1 || !W || !D_inout || !Ds_out || !Gold_out) { set_error("op_lrr_direction: invalid argument"); return CUADMM_ERR_INVALID; }
  int rc = lrr_device();
  if (rc) return rc;
  DevBuf<double> buf[4];
  double* dev[4];
  double* const dst[4] = {nullptr, D_inout, Ds_out, Gold_out};
  const double* const src[4] = {W, D_inout, Ds_out, Gold_out};
  const long long len[4] = {n, n + 1, n + 1, n + 1};
  if ((rc = lrr_stage(4, src, len, buf, dev))) return rc;
  if ((rc = launch_lrr_direction(n, dev[0], unit, beta, restart, root, dev[1], dev[2], dev[3], nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  for (int v = 1; v < 4; ++v)
    if ((rc = staged_d2h(dst[v], dev[v], sizeof(double) * (size_t)len[v]))) return rc;
  return CUADMM_OK;
}
// L_inout, Ls_out: n + 1 doubles each (the guard last); D: n
int cuadmm_op_lrr_step(long long n, double t, double root, const double* D, double* L_inout, double* Ls_out) {
  if (n < 1 || !D || !L_inout || !Ls_out) { set_error("op_lrr_step: invalid argument"); return CUADMM_ERR_INVALID; }
  int rc = lrr_device();
  if (rc) return rc;
  DevBuf<double> buf[3];
  double* dev[3];
  double* const dst[3] = {nullptr, L_inout, Ls_out};
  const double* const src[3] = {D, L_inout, Ls_out};
  const long long len[3] = {n, n + 1, n + 1};
  if ((rc = lrr_stage(3, src, len, buf, dev))) return rc;
  if ((rc = launch_lrr_step(n, t, root, dev[0], dev[1], dev[2], nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  for (int v = 1; v < 3; ++v)
    if ((rc = staged_d2h(dst[v], dev[v], sizeof(double) * (size_t)len[v]))) return rc;
  return CUADMM_OK;
}

// cuadmm_set_lowrank's, cuadmm_block_multiply's, cuadmm_lowrank_grad's, cuadmm_lowrank_line's and cuadmm_lowrank_refine's check of the caller's factors
// (csrc/factor_layout.h: check_factors) under the name `who`, with the buffers named as that call names them: "V" for block_multiply, else
// "L", and "D" beside it for lowrank_line (D is not looked at for the others).  Host only.
int cuadmm_op_check_factors(const char* who, const int* blk_vals, int mat_num, const int* ranks, int rmax, const double* L, const double* D) {
  if (!who || !blk_vals || mat_num < 1) { set_error("op_check_factors: invalid argument"); return CUADMM_ERR_INVALID; }
  const bool two = !std::strcmp(who, "lowrank_line");
  return check_factors(who, mat_num, blk_vals, ranks, rmax, std::strcmp(who, "block_multiply") ? "L" : "V", L, two ? "D" : nullptr, two ? D : nullptr, nullptr, nullptr);
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
