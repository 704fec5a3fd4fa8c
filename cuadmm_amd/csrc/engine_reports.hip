// What the engine reports beside the iteration: the infeasibility check and the certified lower bound behind the iteration's steps, and
// the reports on a point (cuadmm_lower_bound, cuadmm_evaluate, cuadmm_lambda_min, cuadmm_lowrank, cuadmm_block_multiply,
// cuadmm_lowrank_grad, cuadmm_lowrank_line, cuadmm_lowrank_refine) with their C entry points.  Host code only: the kernels are those of
// infeas.hip, lower_bound.hip, evaluate.hip, lambda_min.hip, lowrank.hip, lowrank_apply.hip, block_mult.hip, lowrank_grad.hip,
// lowrank_line.hip, lowrank_refine.hip and the iteration's own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "engine_state.h"

using namespace cuadmm;

// ------------------------------------------------------------------------------------------
// Infeasibility detection (option "infeas_check"): DESIGN.md, "Infeasibility certificates"
// ------------------------------------------------------------------------------------------
// Auxiliary projector (infeasibility check, lower bound)
int AuxProj::ensure(cuadmm_solver& s) {
  int rc;
  if (!ev[1]) {
    if ((rc = in.alloc((size_t)s.L)) || (rc = out.alloc((size_t)s.L)) || (!s.b_d.p && (rc = bcopy.alloc((size_t)std::max(s.m, 1))))) return rc;
    for (auto& e : ev) if ((rc = e.create())) return rc;
  }
  if (bcopy.p && s.m > 0 && (rc = staged_h2d(bcopy.p, s.b_p.data(), sizeof(double) * (size_t)s.m, s.st))) return rc;
  return CUADMM_OK;
}
int AuxProj::project(cuadmm_solver& s, const double* from, double* to) {
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
    o[3] = slot_sum(h + kLmOut * (size_t)nb) * objscale - pen;
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

// ------------------------------------------------------------------------------------------
// Blocks times factors (cuadmm_block_multiply): DESIGN.md, "Blocks times factors"
// ------------------------------------------------------------------------------------------
// the factor layout for this rmax; task list and events on first use, larger buffers when the layout grew; for which = 2 the y vector
// and the auxiliary projector's vectors
int cuadmm_solver::bm_prepare(int which, int rmax) {
  int rc;
  const int nb = (int)blk_local.size();
  if (!btasks.built && (rc = btasks.build(blk_local.data(), nb, nullptr))) return rc;
  if ((rc = fl.prepare(blk_local.data(), nb, rmax)) || (rc = bm.prepare(fl, blk_local.data()))) return rc;
  if (which != 2) return CUADMM_OK;
  if (!bm.ybuf.p && (rc = bm.ybuf.alloc((size_t)std::max(m, 1)))) return rc;
  return aux.ensure(*this);
}

// which = 0: X, 1: S, read where they lie (scaled behind a solve, else in the caller's units); 2: S^ = C - A'y at the scaled y in bm.ybuf,
// formed as -(A'y - C) by the iteration's kernel into the auxiliary projector's input vector (the launch of dual_slack without its b'y
// sums, which nothing here reads: the timed interval is that launch and the product).  The kernel's W is in the units of
// the vector it read and goes to the caller's on the host, one multiplication per entry.  The norms and inner products are plain double
// sums over the returned W and the caller's V in index order (no contraction: a caller reproduces them bit for bit).  Writes only the
// plan's own buffers and that input vector.
int cuadmm_solver::bm_run(int which, const double* V, const int* ranks, double* W_out, double o[8], double* per_block) {
  int rc;
  const int nb = (int)blk_local.size();
  const double* v = which == 0 ? X.p : S.p;
  double sign = 1.0, unit = pending_unscale ? (which == 0 ? bscale : Cscale) : 1.0;
  if ((rc = fl.stage(bm.Vbuf, V)) || (rc = fl.stage_ranks(ranks))) return rc;
  CUADMM_HIP_TRY(hipEventRecord(bm.ev[0], st));
  if (which == 2) {
    if ((rc = launch_aty_xb(false, L, At_rp.p, At_ci.p, At_v.p, bm.ybuf.p, C.p, X.p, 1.0, aux.in.p, nullptr, st, &At_long))) return rc;
    v = aux.in.p; sign = -1.0; unit = Cscale;
  }
  if ((rc = bm.run(fl, v, sign, btasks.off.p, btasks.blk.p, st))) return rc;
  CUADMM_HIP_TRY(hipEventRecord(bm.ev[1], st));
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  const float ms = event_ms(bm.ev[0], bm.ev[1]);
  bm.calls++;
  if ((rc = bm.fetch(fl, blk_local.data(), ranks, unit, W_out))) return rc;
  double sq_all = 0, dot_all = 0, best = 0, blocks = 0, rank_sum = 0;
  int arg = -1;
  for (int k = 0; k < nb; ++k) {
    const int n = blk_local[k];
    double sq = 0, dot = 0, vsq = 0;
    if (n > 0) {
#pragma clang fp contract(off)
      const double *w = W_out + fl.loff[k], *x = V ? V + fl.loff[k] : nullptr;
      for (size_t e = 0, used = (size_t)n * (size_t)ranks[k]; e < used; ++e) {
        const double ww = w[e] * w[e], vw = x[e] * w[e], vv = x[e] * x[e];
        sq = sq + ww; dot = dot + vw; vsq = vsq + vv;
      }
      sq_all = sq_all + sq; dot_all = dot_all + dot;
      blocks += 1; rank_sum += ranks[k];
      const double nrm = std::sqrt(sq);
      if (arg < 0 || nrm > best) { best = nrm; arg = k; }
    }
    if (per_block) {
      double* q = per_block + 4 * (size_t)k;
      q[0] = std::sqrt(sq); q[1] = dot; q[2] = std::sqrt(vsq); q[3] = n > 0 ? 0.0 : 2.0;
    }
  }
  o[0] = std::sqrt(sq_all); o[1] = dot_all; o[2] = (double)arg; o[3] = best; o[4] = blocks; o[5] = rank_sum;
  o[6] = ms;
  o[7] = bm.bytes() + fl.bytes() + btasks.bytes() + (bm.ybuf.p ? aux.bytes() : 0.0);
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// Value and gradient at factors (cuadmm_lowrank_grad): DESIGN.md, "Value and gradient at factors"
// ------------------------------------------------------------------------------------------
// the factor layout for this rmax and the two kernels' plans on it, the plan's own vectors on first use; the column norms (where the engine keeps none on the device)
// and the auxiliary projector's vectors and b on every call
int cuadmm_solver::lg_prepare(int rmax) {
  int rc;
  const int nb = (int)blk_local.size();
  if (!btasks.built && (rc = btasks.build(blk_local.data(), nb, nullptr))) return rc;
  if ((rc = fl.prepare(blk_local.data(), nb, rmax)) || (rc = bm.prepare(fl, blk_local.data())) || (rc = lo.prepare(fl, blk_local.data())) ||
      (rc = lg.prepare(L, m, nb, btasks.nchunk, !normA_d.p)))
    return rc;
  if (lg.normA.p && m > 0 && (rc = staged_h2d(lg.normA.p, normA_p.data(), sizeof(double) * (size_t)m, st))) return rc;
  return aux.ensure(*this);
}

// The launches of lg_run's chain at the scaled y in lg.ybuf, on device buffers: Lx the factors in the units X lies in (the outer product
// reads them), bm.Vbuf those in the caller's units (the block product reads them).  The per-block terms only where f is wanted from them.
int cuadmm_solver::lg_enqueue(const double* Lx, double sigma, bool block_terms) {
  int rc;
  const double* const normA_dev = normA_d.p ? normA_d.p : lg.normA.p;
  CUADMM_HIP_TRY(hipMemcpyAsync(lg.xv.p, X.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, st));
  if ((rc = lo.run(fl, Lx, btasks.off.p, btasks.blk.p, lg.xv.p, st))) return rc;
  if (m > 0 && (rc = launch_spmv_rows(m, A_avg_nnz, A_rp.p, A_ci.p, A_v.p, lg.xv.p, S.p, C.p, lg.ax.p, nullptr, st, &A_long))) return rc;
  if ((rc = launch_lrg_multiplier(m, lg.ax.p, aux.b_dev(*this), normA_dev, lg.ybuf.p, pending_unscale ? 1.0 : 1 / bscale, bscale, 1 / Cscale, sigma, lg.ytilde.p,
                                  lg.r.p, lg.part.p, st)))
    return rc;
  if ((rc = launch_aty_xb(false, L, At_rp.p, At_ci.p, At_v.p, lg.ytilde.p, C.p, X.p, 1.0, aux.in.p, nullptr, st, &At_long))) return rc;
  if ((rc = bm.run(fl, aux.in.p, -1.0, btasks.off.p, btasks.blk.p, st))) return rc;
  if (block_terms && (rc = launch_lrg_block_terms(C.p, lg.xv.p, aux.in.p, btasks.view(), lg.cpart.p, lg.sums.p, st))) return rc;
  return CUADMM_OK;
}

// The chain at the scaled y in lg.ybuf.  x is assembled in lg.xv in the units X lies in (X = ux xv: ux = bscale behind a solve, else 1): a
// device copy of X, then svec(L_k L_k') over its PSD blocks from the factors in those units -- the caller's own, as the block product's V
// holds them, where ux = 1, else a second staged copy through scale_factors.  Then A x, the multiplier pass, M = A'ytilde - C into the
// auxiliary projector's input vector (S^ = -Cscale M), W = -M_k L_k with the caller's L (the launch and the unit of
// cuadmm_block_multiply(2): sigma = 0 gives its bits) and the per-block terms.  G = 2 (Cscale W), the doubling exact.  The sums over G and L
// are plain double sums in index order, as in bm_run.  Reads X, y, A, A', b, C; writes only the plans' own buffers and that input vector.
int cuadmm_solver::lg_run(const double* Lf, const int* ranks, double sigma, double* G_out, double* r_out, double* Shat_out, double o[8], double* per_block) {
  int rc;
  const int nb = (int)blk_local.size();
  const double ux = pending_unscale ? bscale : 1.0;
  if ((rc = fl.stage(bm.Vbuf, Lf)) || (rc = fl.stage_ranks(ranks))) return rc;
  const double* Lx = bm.Vbuf.p;
  if (ux != 1.0 && Lf) {
    scale_factors(fl, blk_local.data(), ranks, Lf, ux, lg.h_stage);      // (kept by the plan: a caller's optimiser makes this call in a loop)
    if ((rc = fl.stage(lo.Lbuf, lg.h_stage.data()))) return rc;
    Lx = lo.Lbuf.p;
  }
  CUADMM_HIP_TRY(hipEventRecord(lg.ev[0], st));
  if ((rc = lg_enqueue(Lx, sigma, true))) return rc;
  CUADMM_HIP_TRY(hipEventRecord(lg.ev[1], st));
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  const float ms = event_ms(lg.ev[0], lg.ev[1]);
  // --- back to the host and to the caller's units (the host scratch is the plan's and is kept)
  std::vector<double>& h = lg.h_back;
  h.resize((size_t)std::max(m, 1) + 2 * (size_t)kBrSlots + kLgSums * (size_t)nb);
  if (!G_out) { lg.h_G.resize(fl.count() + 1); G_out = lg.h_G.data(); }
  if ((rc = bm.fetch(fl, blk_local.data(), ranks, Cscale, G_out))) return rc;
  double *const rh = h.data(), *const part = rh + std::max(m, 1), *const sums = part + 2 * kBrSlots;
  if (m > 0 && (rc = staged_d2h(rh, lg.r.p, sizeof(double) * (size_t)m, st))) return rc;
  if ((rc = staged_d2h(part, lg.part.p, sizeof(double) * 2 * kBrSlots, st))) return rc;
  if (nb > 0 && (rc = staged_d2h(sums, lg.sums.p, sizeof(double) * kLgSums * (size_t)nb, st))) return rc;
  unpermute(perm, m, rh, r_out);
  if (Shat_out) {
    if ((rc = staged_d2h(Shat_out, aux.in.p, sizeof(double) * (size_t)L, st))) return rc;
    for (long long i = 0; i < L; ++i) Shat_out[i] = -(Shat_out[i] * Cscale);
  }
  double cx = 0, sq_all = 0, dot_all = 0;
  const double yr = slot_sum(part) * objscale, rn2 = slot_sum(part + kBrSlots);
  const double cxu = Cscale * ux;
  for (int k = 0; k < nb; ++k) {
    const int n = blk_local[k];
    const double cxk = sums[kLgSums * (size_t)k] * cxu;
    double sq = 0, dot = 0, lsq = 0;
    if (n > 0) {
#pragma clang fp contract(off)
      double* g = G_out + fl.loff[k];
      const double* x = Lf ? Lf + fl.loff[k] : nullptr;
      for (size_t e = 0, used = (size_t)n * (size_t)ranks[k]; e < used; ++e) {
        g[e] = 2.0 * g[e];
        const double gg = g[e] * g[e], lg_ = x[e] * g[e], ll = x[e] * x[e];
        sq = sq + gg; dot = dot + lg_; lsq = lsq + ll;
      }
      sq_all = sq_all + sq; dot_all = dot_all + dot;
    }
    cx = cx + cxk;
    if (per_block) {
      double* q = per_block + 4 * (size_t)k;
      q[0] = cxk; q[1] = n > 0 ? std::sqrt(sq) : std::sqrt(sums[kLgSums * (size_t)k + 1]) * Cscale; q[2] = dot; q[3] = lsq;
    }
  }
  o[0] = cx - yr + (0.5 * sigma) * rn2; o[1] = cx; o[2] = yr; o[3] = std::sqrt(rn2); o[4] = std::sqrt(sq_all); o[5] = dot_all;
  o[6] = ms;
  o[7] = lg.bytes() + bm.bytes() + lo.bytes() + fl.bytes() + btasks.bytes() + aux.bytes();
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// The quartic along a line in factor space (cuadmm_lowrank_line): DESIGN.md, "Line search along factor steps"
// ------------------------------------------------------------------------------------------
// the factor layout for this rmax and the outer product's plan on it, the plan's own vectors on first use and a device D that grows with it; the column norms
// (where the engine keeps none on the device) and the auxiliary projector's b on every call
int cuadmm_solver::ll_prepare(int rmax) {
  int rc;
  const int nb = (int)blk_local.size();
  if (!btasks.built && (rc = btasks.build(blk_local.data(), nb, nullptr))) return rc;
  if ((rc = fl.prepare(blk_local.data(), nb, rmax)) || (rc = lo.prepare(fl, blk_local.data())) || (rc = ll.prepare(L, m, nb, btasks.nchunk, !normA_d.p, st)) ||
      (rc = ll.Dbuf.grow(fl.count() + 1)))
    return rc;
  if (ll.normA.p && m > 0 && (rc = staged_h2d(ll.normA.p, normA_p.data(), sizeof(double) * (size_t)m, st))) return rc;
  return aux.ensure(*this);
}

// The launches of ll_run's chain at the scaled y in ll.ybuf, on the factors in lo.Lbuf and the direction in ll.Dbuf, both in the units X
// lies in.
int cuadmm_solver::ll_enqueue() {
  int rc;
  const double* const normA_dev = normA_d.p ? normA_d.p : ll.normA.p;
  CUADMM_HIP_TRY(hipMemcpyAsync(ll.x0.p, X.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, st));
  if ((rc = launch_block_outer3((int)lo.tasks.size(), lo.tasks_d.p, lo.Lbuf.p, ll.Dbuf.p, fl.loff_d.p, fl.ranks_d.p, btasks.off.p, btasks.blk.p, ll.x0.p, ll.x1.p,
                                ll.x2.p, st)))
    return rc;
  if (m > 0) {
    const double* const xs[3] = {ll.x0.p, ll.x1.p, ll.x2.p};
    double* const axs[3] = {ll.ax0.p, ll.ax1.p, ll.ax2.p};
    for (int j = 0; j < 3; ++j)
      if ((rc = launch_spmv_rows(m, A_avg_nnz, A_rp.p, A_ci.p, A_v.p, xs[j], S.p, C.p, axs[j], nullptr, st, &A_long))) return rc;
  }
  if ((rc = launch_lrl_sums(m, ll.ax0.p, ll.ax1.p, ll.ax2.p, aux.b_dev(*this), normA_dev, ll.ybuf.p, pending_unscale ? 1.0 : 1 / bscale, bscale, ll.r0.p, ll.p.p, ll.q.p,
                            ll.part.p, st)))
    return rc;
  return launch_lrl_block_terms(C.p, ll.x0.p, ll.x1.p, ll.x2.p, btasks.view(), ll.cpart.p, ll.sums.p, st);
}

// Behind ll_enqueue: the slot partials and the per-block sums to the plan's host scratch (ll.h_back: three m-vectors for the caller of
// ll_run, then the partials, then the sums; *sums points at the last), sm <- the nine slot sums, c <- the coefficients in the order
// lowrank_line.h states.
int cuadmm_solver::ll_coef(double sigma, double ux, double c[5], double sm[kLlParts], const double** sums_out) {
#pragma clang fp contract(off)
  int rc;
  const int nb = (int)blk_local.size();
  const size_t mm = (size_t)std::max(m, 1);
  std::vector<double>& h = ll.h_back;
  h.resize(3 * mm + kLlParts * (size_t)kBrSlots + kLlSums * (size_t)std::max(nb, 1));
  double *const part = h.data() + 3 * mm, *const sums = part + kLlParts * (size_t)kBrSlots;
  if ((rc = staged_d2h(part, ll.part.p, sizeof(double) * kLlParts * (size_t)kBrSlots, st))) return rc;
  if (nb > 0 && (rc = staged_d2h(sums, ll.sums.p, sizeof(double) * kLlSums * (size_t)nb, st))) return rc;
  double cx[kLlSums] = {0, 0, 0};
  for (int j = 0; j < kLlParts; ++j) sm[j] = slot_sum(part + (size_t)j * kBrSlots);
  const double cxu = Cscale * ux;
  for (int k = 0; k < nb; ++k)
    for (int j = 0; j < kLlSums; ++j) cx[j] = cx[j] + sums[kLlSums * (size_t)k + j] * cxu;
  const double yr0 = sm[0] * objscale, yr1 = sm[1] * objscale, yr2 = sm[2] * objscale, hs = 0.5 * sigma;
  c[0] = (cx[0] - yr0) + hs * sm[3];
  c[1] = (cx[1] - yr1) + sigma * sm[4];
  c[2] = (cx[2] - yr2) + hs * (sm[5] + 2.0 * sm[6]);
  c[3] = sigma * sm[7];
  c[4] = hs * sm[8];
  *sums_out = sums;
  return CUADMM_OK;
}

// The chain at the scaled y in ll.ybuf.  L and D are staged in the units X lies in (X = ux x: ux = bscale behind a solve, else 1), through
// scale_factors where ux != 1 as lg_run stages L, so that x0 and with it r0 carry lg_run's bits.  Then the device copy of X into
// ll.x0, the three outer products, three A x, the streaming pass and the per-block terms; the coefficients on the host in the order
// lowrank_line.h states.  Reads X, A, b, C; writes only the plans' own buffers.  Every output of the caller is written behind the last
// refusal.
int cuadmm_solver::ll_run(const double* Lf, const double* Df, const int* ranks, double sigma, double t_max, double coef5[5], double* r_out, double* p_out,
                          double* q_out, double o[8], double* per_block) {
#pragma clang fp contract(off)
  int rc;
  const int nb = (int)blk_local.size();
  const double ux = pending_unscale ? bscale : 1.0;
  const double *Ls = Lf, *Ds = Df;
  if (ux != 1.0 && Lf) {
    scale_factors(fl, blk_local.data(), ranks, Lf, ux, ll.h_L);
    scale_factors(fl, blk_local.data(), ranks, Df, ux, ll.h_D);
    Ls = ll.h_L.data(); Ds = ll.h_D.data();
  }
  if ((rc = fl.stage(lo.Lbuf, Ls)) || (rc = fl.stage(ll.Dbuf, Ds)) || (rc = fl.stage_ranks(ranks))) return rc;
  CUADMM_HIP_TRY(hipEventRecord(ll.ev[0], st));
  if ((rc = ll_enqueue())) return rc;
  CUADMM_HIP_TRY(hipEventRecord(ll.ev[1], st));
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  const float ms = event_ms(ll.ev[0], ll.ev[1]);
  // --- back to the host and to the caller's units (the host scratch is the plan's and is kept)
  double sm[kLlParts], c[5];
  const double* sums = nullptr;
  if ((rc = ll_coef(sigma, ux, c, sm, &sums))) return rc;
  const size_t mm = (size_t)std::max(m, 1);
  double *const rh = ll.h_back.data(), *const ph = rh + mm, *const qh = ph + mm;
  if (m > 0 && r_out && (rc = staged_d2h(rh, ll.r0.p, sizeof(double) * (size_t)m, st))) return rc;
  if (m > 0 && p_out && (rc = staged_d2h(ph, ll.p.p, sizeof(double) * (size_t)m, st))) return rc;
  if (m > 0 && q_out && (rc = staged_d2h(qh, ll.q.p, sizeof(double) * (size_t)m, st))) return rc;
  const double cxu = Cscale * ux;
  double q4[4] = {0.0, c[0], 0.0, 0.0};
  if (t_max > 0.0) {
    for (int j = 0; j < 5; ++j)
      if (!std::isfinite(c[j])) { set_error("lowrank_line: c%d = %g is not finite", j, c[j]); return CUADMM_ERR_INVALID; }
    if ((rc = cuadmm_quartic_min(c, t_max, q4))) return rc;
  }
  // --- nothing is refused from here on
  for (int j = 0; j < 5; ++j) coef5[j] = c[j];
  unpermute(perm, m, rh, r_out);
  unpermute(perm, m, ph, p_out);
  unpermute(perm, m, qh, q_out);
  for (int k = 0; per_block && k < nb; ++k) {
    double* w = per_block + 4 * (size_t)k;
    for (int j = 0; j < kLlSums; ++j) w[j] = sums[kLlSums * (size_t)k + j] * cxu;
    w[3] = blk_local[k] > 0 ? 0.0 : 2.0;
  }
  o[0] = q4[0]; o[1] = q4[1]; o[2] = q4[2]; o[3] = std::sqrt(sm[5]); o[4] = std::sqrt(sm[8]); o[5] = q4[3];
  o[6] = ms;
  o[7] = ll.bytes() + lo.bytes() + fl.bytes() + btasks.bytes() + aux.bytes();
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// Conjugate gradients over the factors (cuadmm_lowrank_refine): DESIGN.md, "Refinement over factors"
// ------------------------------------------------------------------------------------------
// what cuadmm_lowrank_grad and cuadmm_lowrank_line prepare for this rmax, and the loop's own buffers on the same layout
int cuadmm_solver::rf_prepare(int rmax) {
  int rc;
  if ((rc = lg_prepare(rmax)) || (rc = ll_prepare(rmax))) return rc;
  return rf.prepare(fl);
}

// `steps` steps of Polak-Ribiere+ conjugate gradients at the scaled y in lg.ybuf and ll.ybuf (the same bits).  Resident between the steps:
// L in the caller's units in bm.Vbuf (the block product reads it) and in the units X lies in in lo.Lbuf (both outer products read it), the
// direction in the caller's units in rf.D and scaled in ll.Dbuf, the block product's W in bm.Wbuf (G = 2 (Cscale W) wherever it is read)
// and the previous G in rf.Gold.  A step enqueues lg_run's chain without the per-block terms, the three sums, the direction, ll_run's
// chain and the update of L, and synchronises twice: for the three sums and for the quartic's partials.  The host packs the caller's L
// into a clean buffer first (+ 0.0 in the columns that are not read) and zeroes W, D and G_old once: the block product never writes
// the columns >= r_k, so the flat kernels see zeros there throughout.  Every output of the caller is written at the end.
// Reads X, y, A, A', b, C; writes only the plans' own buffers and the auxiliary projector's input vector.
int cuadmm_solver::rf_run(const double* Lf, const int* ranks, double sigma, int steps, double t_max, double gtol, double* L_out, double* trace, double o[8],
                          double* r_out) {
#pragma clang fp contract(off)
  int rc;
  const int nb = (int)blk_local.size();
  const size_t count = fl.count();
  const long long cnt = (long long)count;
  const double ux = pending_unscale ? bscale : 1.0, root = 1 / std::sqrt(ux);
  std::vector<double>& hL = rf.h_L;
  hL.assign(count + 1, 0.0);
  for (int k = 0; k < nb; ++k)
    for (size_t e = (size_t)fl.loff[k], end = e + (blk_local[k] > 0 ? (size_t)blk_local[k] * (size_t)ranks[k] : 0); e < end; ++e) hL[e] = Lf[e];
  scale_factors(fl, blk_local.data(), ranks, hL.data(), ux, lg.h_stage);
  if ((rc = fl.stage(bm.Vbuf, hL.data())) || (rc = fl.stage(lo.Lbuf, lg.h_stage.data())) || (rc = fl.stage_ranks(ranks))) return rc;
  if (count > 0) {
    CUADMM_HIP_TRY(hipMemsetAsync(bm.Wbuf.p, 0, sizeof(double) * count, st));
    CUADMM_HIP_TRY(hipMemsetAsync(rf.D.p, 0, sizeof(double) * count, st));
    CUADMM_HIP_TRY(hipMemsetAsync(rf.Gold.p, 0, sizeof(double) * count, st));
  }
  std::vector<double> tr((size_t)kRfTrace * (size_t)steps, 0.0);
  std::vector<double>& hp = rf.h_part;
  hp.resize(kRfParts * (size_t)kBrSlots);
  double gg_prev = 0, first_c0 = NAN, last_f = NAN, last_gn = NAN;
  int taken = 0, reason = 0, rows = 0;
  hipEvent_t prev0 = nullptr, prev1 = nullptr;
  CUADMM_HIP_TRY(hipEventRecord(rf.ev[0], st));
  for (int k = 0; k < steps; ++k) {
    double* const row = tr.data() + (size_t)kRfTrace * (size_t)k;
    hipEvent_t e0 = rf.ev[2 + 2 * (k & 1)], e1 = rf.ev[3 + 2 * (k & 1)];
    rows = k + 1;
    CUADMM_HIP_TRY(hipEventRecord(e0, st));
    // --- the gradient at L_k and the three sums
    if ((rc = lg_enqueue(lo.Lbuf.p, sigma, false))) return rc;
    if ((rc = launch_lrr_dots(cnt, bm.Wbuf.p, Cscale, rf.Gold.p, rf.D.p, rf.part.p, st))) return rc;
    if ((rc = staged_d2h(hp.data(), rf.part.p, sizeof(double) * hp.size(), st))) return rc;      // (drains the stream: the step before is over)
    if (prev0) tr[(size_t)kRfTrace * (size_t)(k - 1) + 13] = event_ms(prev0, prev1);
    prev0 = e0; prev1 = e1;
    const double gg = slot_sum(hp.data()), go = slot_sum(hp.data() + kBrSlots), gd = slot_sum(hp.data() + 2 * (size_t)kBrSlots);
    row[0] = gg; row[1] = go; row[2] = gd;
    last_gn = std::sqrt(gg);
    double u3[3];
    if (!std::isfinite(gg) || !std::isfinite(go) || !std::isfinite(gd) || cuadmm_cg_update(gg, go, gd, gg_prev, k == 0, u3)) { reason = 3; CUADMM_HIP_TRY(hipEventRecord(e1, st)); break; }
    row[3] = u3[0]; row[4] = u3[1]; row[5] = u3[2];
    if (gtol > 0.0 && last_gn <= gtol) { reason = 2; CUADMM_HIP_TRY(hipEventRecord(e1, st)); break; }
    // --- the direction and the quartic along it
    if ((rc = launch_lrr_direction(cnt, bm.Wbuf.p, Cscale, u3[0], u3[2] != 0.0, root, rf.D.p, ll.Dbuf.p, rf.Gold.p, st))) return rc;
    if ((rc = ll_enqueue())) return rc;
    double c[5], sm[kLlParts], q4[4];
    const double* sums = nullptr;
    if ((rc = ll_coef(sigma, ux, c, sm, &sums))) return rc;
    for (int j = 0; j < 5; ++j) row[6 + j] = c[j];
    if (k == 0) first_c0 = c[0];
    bool finite = true;
    for (int j = 0; j < 5; ++j) finite = finite && std::isfinite(c[j]);
    if (!finite) { reason = 3; CUADMM_HIP_TRY(hipEventRecord(e1, st)); break; }
    if (cuadmm_quartic_min(c, t_max, q4)) { reason = 4; CUADMM_HIP_TRY(hipEventRecord(e1, st)); break; }
    row[11] = q4[0]; row[12] = q4[1];
    last_f = q4[1];
    if (q4[0] == 0.0) { reason = 1; CUADMM_HIP_TRY(hipEventRecord(e1, st)); break; }
    // --- the step
    if ((rc = launch_lrr_step(cnt, q4[0], root, rf.D.p, bm.Vbuf.p, lo.Lbuf.p, st))) return rc;
    CUADMM_HIP_TRY(hipEventRecord(e1, st));
    gg_prev = gg;
    taken++;
  }
  CUADMM_HIP_TRY(hipEventRecord(rf.ev[1], st));
  CUADMM_HIP_TRY(hipStreamSynchronize(st));
  if (prev0) tr[(size_t)kRfTrace * (size_t)(rows - 1) + 13] = event_ms(prev0, prev1);
  const float ms = event_ms(rf.ev[0], rf.ev[1]);
  rf.calls++;
  // --- back to the host: L in the caller's units (its columns >= r_k have stayed + 0.0), r of the last gradient chain (the bits of the
  // line search's r0 at the same factors)
  if (count > 0 && (rc = staged_d2h(hL.data(), bm.Vbuf.p, sizeof(double) * count, st))) return rc;
  std::vector<double> rh((size_t)std::max(m, 1));
  if (m > 0 && r_out && (rc = staged_d2h(rh.data(), lg.r.p, sizeof(double) * (size_t)m, st))) return rc;
  // --- nothing fails from here on
  std::copy(hL.begin(), hL.begin() + count, L_out);
  std::copy(tr.begin(), tr.begin() + (size_t)kRfTrace * (size_t)rows, trace);
  unpermute(perm, m, rh.data(), r_out);
  o[0] = (double)taken; o[1] = (double)reason; o[2] = first_c0; o[3] = last_f; o[4] = last_gn; o[5] = ms;
  o[6] = rf.bytes() + lg.bytes() + ll.bytes() + bm.bytes() + lo.bytes() + fl.bytes() + btasks.bytes() + aux.bytes();
  o[7] = 0;
  return CUADMM_OK;
}

extern "C" {

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
  std::vector<long long> loff;
  int rc = factor_offsets("lowrank_size", (int)s->blk_local.size(), s->blk_local.data(), rmax, &loff);
  if (rc) return rc;
  *count_out = loff.back();
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
int cuadmm_block_multiply(cuadmm_solver* s, int which, const double* V, const int* ranks, int rmax, double* W_out, double o[8], double* per_block) {
  int rc = report_guard(s, o, "block_multiply", "results", which == 2);
  if (rc) return rc;
  if (which < 0 || which > 2) { set_error("block_multiply: which = %d (0: X, 1: S, 2: C - A'y)", which); return CUADMM_ERR_INVALID; }
  if (rmax < 1 || rmax > kMaxBlockSize) { set_error("block_multiply: rmax = %d, allowed are 1 to %d", rmax, kMaxBlockSize); return CUADMM_ERR_INVALID; }
  if (!W_out || !ranks) { set_error("block_multiply: W_out or ranks is null"); return CUADMM_ERR_INVALID; }
  if ((rc = check_factors("block_multiply", (int)s->blk_local.size(), s->blk_local.data(), ranks, rmax, "V", V, nullptr, nullptr, nullptr, nullptr))) return rc;
  if ((rc = s->bm_prepare(which, rmax)) || (which == 2 && (rc = s->stage_scaled_y(s->bm.ybuf.p, nullptr)))) return rc;
  return s->bm_run(which, V, ranks, W_out, o, per_block);
}
int cuadmm_lowrank_grad(cuadmm_solver* s, const double* Lf, const int* ranks, int rmax, const double* y, double sigma, double* G_out, double* r_out,
                        double* Shat_out, double o[8], double* per_block) {
  int rc = report_guard(s, o, "lowrank_grad", "results", true);
  if (rc) return rc;
  if (!(sigma >= 0.0) || !std::isfinite(sigma)) { set_error("lowrank_grad: sigma = %g, allowed is a finite sigma >= 0", sigma); return CUADMM_ERR_INVALID; }
  if (rmax < 1 || rmax > kMaxBlockSize) { set_error("lowrank_grad: rmax = %d, allowed are 1 to %d", rmax, kMaxBlockSize); return CUADMM_ERR_INVALID; }
  if (!ranks) { set_error("lowrank_grad: ranks is null"); return CUADMM_ERR_INVALID; }
  if ((rc = check_factors("lowrank_grad", (int)s->blk_local.size(), s->blk_local.data(), ranks, rmax, "L", Lf, nullptr, nullptr, nullptr, nullptr))) return rc;
  for (int i = 0; y && i < s->m; ++i)
    if (!std::isfinite(y[i])) { set_error("lowrank_grad: y[%d] is not finite", i); return CUADMM_ERR_INVALID; }
  if ((rc = s->lg_prepare(rmax)) || (rc = s->stage_scaled_y(s->lg.ybuf.p, y))) return rc;
  return s->lg_run(Lf, ranks, sigma, G_out, r_out, Shat_out, o, per_block);
}
int cuadmm_lowrank_line(cuadmm_solver* s, const double* Lf, const double* Df, const int* ranks, int rmax, const double* y, double sigma, double t_max,
                        double coef5[5], double* r_out, double* p_out, double* q_out, double o[8], double* per_block) {
  int rc = report_guard(s, o, "lowrank_line", "results", true);
  if (rc) return rc;
  if (!coef5) { set_error("lowrank_line: coef5 is null"); return CUADMM_ERR_INVALID; }
  if (!(sigma >= 0.0) || !std::isfinite(sigma)) { set_error("lowrank_line: sigma = %g, allowed is a finite sigma >= 0", sigma); return CUADMM_ERR_INVALID; }
  if (std::isnan(t_max)) { set_error("lowrank_line: t_max is not a number"); return CUADMM_ERR_INVALID; }
  if (rmax < 1 || rmax > kMaxBlockSize) { set_error("lowrank_line: rmax = %d, allowed are 1 to %d", rmax, kMaxBlockSize); return CUADMM_ERR_INVALID; }
  if (!ranks) { set_error("lowrank_line: ranks is null"); return CUADMM_ERR_INVALID; }
  if ((rc = check_factors("lowrank_line", (int)s->blk_local.size(), s->blk_local.data(), ranks, rmax, "L", Lf, "D", Df, nullptr, nullptr))) return rc;
  for (int i = 0; y && i < s->m; ++i)
    if (!std::isfinite(y[i])) { set_error("lowrank_line: y[%d] is not finite", i); return CUADMM_ERR_INVALID; }
  if (!Lf || !Df) Lf = Df = nullptr;     // every rank is 0: neither is read
  if ((rc = s->ll_prepare(rmax)) || (rc = s->stage_scaled_y(s->ll.ybuf.p, y))) return rc;
  return s->ll_run(Lf, Df, ranks, sigma, t_max, coef5, r_out, p_out, q_out, o, per_block);
}
int cuadmm_lowrank_refine(cuadmm_solver* s, const double* Lf, const int* ranks, int rmax, const double* y, double sigma, int steps, double t_max, double gtol,
                          double* L_out, double* trace, double o[8], double* r_out) {
  int rc = report_guard(s, o, "lowrank_refine", "results", true);
  if (rc) return rc;
  if (!L_out || !trace) { set_error("lowrank_refine: L_out or trace is null"); return CUADMM_ERR_INVALID; }
  if (!(sigma >= 0.0) || !std::isfinite(sigma)) { set_error("lowrank_refine: sigma = %g, allowed is a finite sigma >= 0", sigma); return CUADMM_ERR_INVALID; }
  if (steps < 1) { set_error("lowrank_refine: steps = %d, allowed is steps >= 1", steps); return CUADMM_ERR_INVALID; }
  if (!(t_max > 0.0)) { set_error("lowrank_refine: t_max = %g, allowed is t_max > 0 (+inf included)", t_max); return CUADMM_ERR_INVALID; }
  if (!(gtol >= 0.0) || !std::isfinite(gtol)) { set_error("lowrank_refine: gtol = %g, allowed is a finite gtol >= 0", gtol); return CUADMM_ERR_INVALID; }
  if (rmax < 1 || rmax > kMaxBlockSize) { set_error("lowrank_refine: rmax = %d, allowed are 1 to %d", rmax, kMaxBlockSize); return CUADMM_ERR_INVALID; }
  if (!ranks) { set_error("lowrank_refine: ranks is null"); return CUADMM_ERR_INVALID; }
  if ((rc = check_factors("lowrank_refine", (int)s->blk_local.size(), s->blk_local.data(), ranks, rmax, "L", Lf, nullptr, nullptr, nullptr, nullptr))) return rc;
  for (int i = 0; y && i < s->m; ++i)
    if (!std::isfinite(y[i])) { set_error("lowrank_refine: y[%d] is not finite", i); return CUADMM_ERR_INVALID; }
  if ((rc = s->rf_prepare(rmax)) || (rc = s->stage_scaled_y(s->lg.ybuf.p, y)) || (rc = s->stage_scaled_y(s->ll.ybuf.p, y))) return rc;
  return s->rf_run(Lf, ranks, sigma, steps, t_max, gtol, L_out, trace, o, r_out);
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

}  // extern "C"
