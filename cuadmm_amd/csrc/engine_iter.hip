// The ADMM iteration: cuadmm_solve (reference src/solver.cu:355-823) and the methods of struct cuadmm_solver that one pass through its loop
// runs -- the collectives, the y-solve, the launchers of the projection and the vector kernels, several iterations per launch, the
// unscaling behind a solve, acceleration.  Host code only: every kernel is launched through its unit's launch_* function.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "engine_state.h"

using namespace cuadmm;

int cuadmm_solver::comm_allreduce(double* buf, size_t count) {
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

int cuadmm_solver::allreduce_scalars(double* v, int n) {
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

int cuadmm_solver::host_solve(bool in_fused_step) {  // y_p = (P(AA^T+eps I)P^T)^-1 rhs_p
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

int cuadmm_solver::upload_y(bool force) {
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

// solve_next (round 5): the y-solve of the NEXT iteration is enqueued behind this iteration's last kernel BEFORE the host waits --
// and the host then waits for an event recorded in front of it, not for the stream.  The reference solves for y at the top of every
// pass through the loop, the breaking one included (solver.cu:478-500 precede the break), so that solve is never speculative; its only
// host input is sigma, which the caller knows will not change in this iteration's step 5.  The GPU runs the solve (0.2 - 0.4 ms on the
// moment relaxations) while the host goes through the stopping test and enqueues the rest of the next iteration: the idle gap at
// the iteration boundary (kernel trace: the largest one of a latency-bound iteration) is gone.
int cuadmm_solver::fetch_out(size_t first, size_t count, bool solve_next) {
  if (!out_mapped) {
    int rc = do_allreduce(out_d.p + first, count);
    if (rc) return rc;
    if ((dev_scalars || dev_solve) && first == 0) {     // [||Rp||^2, b.y, sum Rd^2, <C,X>] (of this rank -> sum over ranks), on the stream
      // without a collective in between the final stage writes the four scalars straight into the pinned host buffer
      // through its device mapping: the fetch is then a stream synchronisation without a copy command
      double* dst = scalars_dst(h_scal_dev, scal_d.p);
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
    if (!ev_early) { int rc = ev_early.create(hipEventDisableTiming | hipEventReleaseToSystem); if (rc) return rc; }
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

int cuadmm_solver::launch_aty(bool write_xb) {
  prof_begin(K_ATY);
  int rc = launch_aty_xb(write_xb, L, At_rp.p, At_ci.p, At_v.p, y_d.p, C.p, X.p, sig, Rd1.p, Xb.p, st, &At_long);
  prof_end(K_ATY, (write_xb ? 32.0 : 16.0) * (double)L + 4.0 * (double)L);
  return rc;
}

int cuadmm_solver::launch_spmv(bool doX, bool doS, bool after_fused) {
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

int cuadmm_solver::launch_project() {
  prof_begin(K_PSD);
  int rc = plan.project(Xb.p, Xproj.p, st);
  prof_end(K_PSD, 16.0 * (double)L);
  return rc;
}

// Step 2 of a fused iteration: Rd1 / Xb on the rest of the svec, then the projection whose fused blocks also do the
// post step `mode` (0: S, X, sums; 1: S only) on their own ranges, then the post step on the rest (+ the sums).
int cuadmm_solver::launch_fused_step(int mode, double tau, int iters) {
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
    double* dst = scalars_dst(bt.h_dev, bt.scal_d.p);
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
    double* dst = scalars_dst(h_scal_dev, scal_d.p);
    if (!quad_seg.p && reduce_quads_segments(nparts, plan.fused_blocks()) > 1 && (rc = quad_seg.alloc(4 * (size_t)reduce_quads_segments(nparts, plan.fused_blocks()) + 4))) return rc;
    rc = launch_reduce_quads(partials.p, nparts, closed.partials2.p, plan.fused_blocks(), dst, out_w + (size_t)m, quad_seg.p, st);
  }
  prof_end(K_POST, (mode == 0 ? 48.0 : 32.0) * (double)plan.n_rest);
  return rc;
}

int cuadmm_solver::launch_post_mode(int mode, double tau) {
  prof_begin(K_POST);
  int rc = launch_post(mode, L, Xproj.p, Rd1.p, C.p, X.p, S.p, 1 / sig, tau * sig, partials.p, out_w + (size_t)m, st);
  prof_end(K_POST, (mode == 0 ? 48.0 : (mode == 1 ? 32.0 : 40.0)) * (double)L);
  return rc;
}

// --- several iterations per launch ---------------------------------------------------------------------------------
bool cuadmm_solver::can_batch() const {
  return can_batch_local() && bt.peers_agree && aa.mem == 0 && inf.period == 0 && lb.period == 0;
}
bool cuadmm_solver::can_batch_local() const {
  return bt.max_iters >= 2 && fuse && closed.active && dev_solve && !lead.ready && plan.n_rest == 0 && eig_rank == 0 && !out_mapped &&
         plan.fused_blocks() > 0 && (bt.allow_mixed || plan.one_dominant_geometry());
}

// Ranks must take the batching decision TOGETHER: it decides which collective a rank issues (shards of a heterogeneous problem
// can differ: no dominant geometry on one, a block with more than 8 rows on another, no blocks at all on a third).  One small
// all-reduce at the start of every solve (options may have changed since the last one).
int cuadmm_solver::batch_agree() {
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

int cuadmm_solver::batch_alloc() {
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

int cuadmm_solver::batch_copy(bool save) {   // checkpoint of everything an iteration reads and writes: X, S, y, [A X | sums | A (S - C)]
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
int cuadmm_solver::batch_rollback(int keep) {
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
    if (profile) for (auto& e : aa.ev) if ((rc = e.create())) return rc;
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
  if (timed) aa.ms += event_ms(aa.ev[0], aa.ev[1]);
  const double gnorm2 = aa.h_dots.p[2 * kAccelMaxMem];

  if (was_pending) {
    aa.pending = false;
    const bool reject = !(aa.safeguard > 0) || !(std::sqrt(gnorm2) <= aa.safeguard * std::sqrt(aa.gnorm2_prev));
    if (reject) return accel_reject();
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
  return accel_candidate(cols_new, gnorm2);
}

// a rejected candidate: back to f_k, bit for bit: X, S, y, the fetched vectors, the scalars of the stopping test.  The wasted iteration stays recorded.
int cuadmm_solver::accel_reject() {
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

// the next iteration starts from a candidate: least squares over the columns held, the fallback saved beside fbuf, the combination into X, S
int cuadmm_solver::accel_candidate(int cols_new, double gnorm2) {
  int rc;
  const size_t n2 = 2 * (size_t)aa.hs;
  const bool timed = profile != 0 && aa.ev[0];
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
  if (timed) aa.ms += event_ms(aa.ev[2], aa.ev[3]);
  aa.pending = true;
  aa.taken++;
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// SDPSolver::solve, in steps.  SolveRun: the arguments of one call (the switch to ADMM changes sig_update_stage_2 and sigscale mid-solve)
// and the decisions of the iteration under way, which one step takes and the next ones read.
// ------------------------------------------------------------------------------------------
struct SolveRun {
  int max_iter;
  double stop_tol;
  int sig_update_threshold, sig_update_stage_1, sig_update_stage_2, switch_admm;
  double sigscale;
  int if_first;
  bool verbose = false;
  int iter = 0;
  double tau = 0;
  bool snapshot = false, sig_may_change = false, from_batch = false, solve_next_ok = false, breakyes = false;
  std::string final_msg;
  // iteration i may change sigma in its step 5 (with the sig_update_stage_2 of NOW: the switch to ADMM halves it)
  bool sig_may_change_at(int i) const {
    return (i <= sig_update_threshold && i % sig_update_stage_1 == 1) || (i > sig_update_threshold && i % sig_update_stage_2 == 1);
  }
};

// lost row exchanges of the four-workgroups-per-row tail kernel (TailSolve::take_failure) are the solve's error; iter > 0: seen in that iteration's sums
static int tail_failure(Solver* s, int iter) {
  const int tf = s->tail.take_failure(s->st);
  if (tf == 0) return CUADMM_OK;
  char at[32] = "";
  if (iter > 0) snprintf(at, sizeof at, " at iteration %d", iter);
  set_error("solve: the dense tail of the A*A^T solve lost %d row exchanges%s (workgroups of a row not co-resident for seconds): y is not valid%s", tf, at,
            iter > 0 ? "; the handle now uses the two-pass tail kernels" : "");
  return CUADMM_ERR_FACTOR;
}

static int solve_begin(Solver* s, SolveRun& r) {
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
  r.verbose = s->verbose && s->rank == 0;
  s->info_iter_num = 0;

  if (r.verbose) {
    printf("\n -------------------------------------------------------------------------------");
    printf("\n                                    cuADMM");
    printf("\n -------------------------------------------------------------------------------");
    printf("\n norm of C = %2.1e, norm of b = %2.1e\n", s->norm_Corg, s->norm_borg);
  }

  if (r.if_first && s->pending_unscale && (rc = s->materialise())) return rc;   // the reference's X, y, S are unscaled after a solve
  if (!r.if_first && s->pending_unscale) {
    // the previous solve left X, y, S scaled and [A X | A (S - C)], Rp as its last iteration formed them: nothing to redo
    s->pending_unscale = false;
  } else if (!r.if_first) {   // solver.cu:385-409: X,y,S currently hold UNSCALED values
    if ((rc = s->sync_y_host())) return rc;
    for (int i = 0; i < m; ++i) s->y_p[i] = (s->y_p[i] * s->normA_p[i]) * (1 / s->Cscale);
    if (s->dev_solve && (rc = s->upload_y(true))) return rc;
    if ((rc = launch_scale(s->X.p, L, 1 / s->bscale, s->st))) return rc;
    if ((rc = launch_scale(s->S.p, L, 1 / s->Cscale, s->st))) return rc;
    if ((rc = s->launch_spmv(true, true))) return rc;
    if ((rc = s->fetch_out(0, 2 * (size_t)m + 2))) return rc;
    s->refresh_Rp();
  }

  if (r.verbose) {
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
  if (s->sw.lpt == 0) s->lpt_next = 0;         // (lpt_next counts iterations over all solve calls of this solver)
  return CUADMM_OK;
}

// ---- Step 0 (solver.cu:419-467): the verdict, the table row and, on the breaking pass, the footer and the way back from a batch
static int stop_test(Solver* s, SolveRun& r) {
  const int iter = r.iter;
  if (std::max(s->maxfeas, s->relgap) < r.stop_tol) { r.breakyes = true; r.final_msg = "Solver ended: converged."; }
  if (iter > r.max_iter) { r.breakyes = true; r.final_msg = "Solver ended: maximum iteration reached"; }
  if (s->solve_status == 5) {           // the certified gap behind the previous iteration (lb_step)
    r.breakyes = true;
    char msg[160];
    snprintf(msg, sizeof msg, "Solver ended: certified gap %.3e (lower bound %.10e at iteration %d)", s->lb.last_g, s->lb.last_lb, s->solve_status_iter);
    r.final_msg = msg;
  } else if (s->solve_status >= 3) {    // a certificate behind the previous iteration (infeas_step)
    r.breakyes = true;
    char msg[128];
    snprintf(msg, sizeof msg, "Solver ended: %s infeasible (certificate at iteration %d)", s->solve_status == 3 ? "primal" : "dual", s->solve_status_iter);
    r.final_msg = msg;
  } else if (r.breakyes) {
    s->solve_status = iter > r.max_iter ? 2 : 1;
    s->solve_status_iter = iter - 1;
  }
  const double seconds = wall_s() - s->t_init0;
  if (r.verbose && (r.breakyes || (iter <= 200 && iter % 50 == 1) || (iter > 200 && iter % 100 == 1))) {
    printf(" %4d | %3.2e %3.2e | %- 5.4e %- 5.4e %3.2e | %5.1f | %2.1e |", iter - 1, s->errRp, s->errRd, s->pobj,
           s->dobj, s->relgap, seconds, s->sig);
    std::cout << std::endl;
  }
  if (!r.breakyes) return CUADMM_OK;
  if (r.verbose) {
    printf("\n -------------------------------------------------------------------------------\n\n");
    std::cout << r.final_msg << std::endl;
    printf("\n primal infeasibility = %2.1e \n dual   infeasibility = %2.1e \n relative gap         = %2.1e", s->errRp,
           s->errRd, s->relgap);
    printf("\n primal objective = %- 9.8e \n dual   objective = %- 9.8e", s->pobj, s->dobj);
    printf("\n\n time per iteration = %2.4fs \n total time         = %2.1fs", seconds / iter, seconds);
    printf("\n -------------------------------------------------------------------------------\n\n");
  }
  s->total_time = wall_s() - s->t_init0;
  // the device is ahead of the host schedule by the unconsumed iterations of a batch: back to the accepted state
  return s->bt.len > 0 ? s->batch_rollback(s->bt.pos) : CUADMM_OK;
}

// the breaking pass, solver.cu:567-576: the best iterate of the ADMM phase is what the solve returns
static int restore_best(Solver* s, const SolveRun& r) {
  if (r.iter > r.switch_admm && s->have_best && s->solve_status < 3) {   // (a certificate describes the last iterate: no restore)
    CUADMM_HIP_TRY(hipMemcpyAsync(s->X.p, s->X_best.p, sizeof(double) * (size_t)s->L, hipMemcpyDeviceToDevice, s->st));
    CUADMM_HIP_TRY(hipMemcpyAsync(s->S.p, s->S_best.p, sizeof(double) * (size_t)s->L, hipMemcpyDeviceToDevice, s->st));
    CUADMM_HIP_TRY(hipStreamSynchronize(s->st));
    if (s->dev_solve) CUADMM_HIP_TRY(hipMemcpy(s->y_d.p, s->y_best_d.p, sizeof(double) * (size_t)s->m, hipMemcpyDeviceToDevice));
    else std::copy(s->y_best_p.begin(), s->y_best_p.end(), s->y_p.begin());   // in place: y_p's storage is page-locked
    if (r.verbose) printf("best max KKT residual after switch  = %2.1e \n", s->best_KKT);
  }
  return CUADMM_OK;
}

// ---- Step 2 (solver.cu:514-656).  The host-side decisions of this iteration (tau, snapshot) depend only on the previous
// iteration's scalars, so they are taken first: the fused projection needs to know which post step follows it.
static int plan_iteration(Solver* s, SolveRun& r) {
  r.tau = (r.iter < r.switch_admm) ? 1.95 : 1.618;                     // solver.cu:747-754
  if (s->errRd < r.stop_tol) r.tau = std::max(1.618, r.tau / 1.1);

  // does this iteration snapshot the iterate between the S update and the X update?
  r.snapshot = false;
  if (r.iter == r.switch_admm) {                                       // solver.cu:681-690
    if (r.verbose) std::cout << " switching to normal ADMM!" << std::endl;
    r.sig_update_stage_2 = r.sig_update_stage_2 / 2;
    if (r.sig_update_stage_2 < 1) r.sig_update_stage_2 = 1;
    r.sigscale = r.sigscale * 1.23;
    s->sgs_KKT = std::max(s->maxfeas, s->relgap);
    s->best_KKT = s->sgs_KKT;
    r.snapshot = true;
  } else if (r.iter > r.switch_admm && s->have_best && !s->aa.pending && s->best_KKT > std::max(s->maxfeas, s->relgap)) {
    // (not in an iteration that started from a candidate of the acceleration: X, y, S there are not the iterate the scalars describe)
    s->best_KKT = std::max(s->maxfeas, s->relgap);                     // solver.cu:732-741
    r.snapshot = true;
  }
  r.sig_may_change = r.sig_may_change_at(r.iter);
  return CUADMM_OK;
}

// ---- several iterations in one launch (SignFuse::iters): ADMM phase without best-iterate bookkeeping, every block closed.
// A batch ends at the next iteration that may change sigma; tau changes only through the errRd < stop_tol rule, checked
// here on every consumed iteration.  Leaves from_batch (this iteration's scalars wait in bt.h) and solve_next_ok.
static int batch_begin(Solver* s, SolveRun& r) {
  int rc;
  if (s->bt.len > 0 && r.tau != s->bt.tau) {
    // this iteration was run with the wrong step length: keep the consumed ones, continue one launch at a time
    if ((rc = s->batch_rollback(s->bt.pos))) return rc;
  }
  if (s->bt.len == 0 && r.iter > r.switch_admm && !s->have_best && !r.snapshot && s->can_batch()) {
    if ((rc = s->batch_alloc())) return rc;
    int K = std::min(std::min(s->bt.max_iters, s->bt.cap), r.max_iter - r.iter + 1);
    for (int j = 0; j < K; ++j) {          // the batch may END on a sigma-update iteration, not contain one
      if (r.sig_may_change_at(r.iter + j)) { K = j + 1; break; }
    }
    if (K >= 2) {
      // a batch can only be invalidated by the stopping test or the errRd < stop_tol rule for tau: no checkpoint without a tolerance
      s->bt.have_ck = r.stop_tol > 0.0;
      if (s->bt.have_ck && (rc = s->batch_copy(true))) return rc;
      s->bt.tau = r.tau; s->bt.sig = s->sig;
      // longest block first without a stall: the step counts are fetched behind one batch; the next one is launched in the new
      // order (the copy of the sorted descriptors is queued on the stream ahead of the launch; the host sort takes ~0.1 ms)
      const bool lpt_sorted_now = s->lpt_next > 0 && s->steps_d.p && s->lpt_steps_ready;
      if (lpt_sorted_now) {
        if ((rc = s->plan.reorder_by_steps_async(s->steps_pin.p, s->st))) return rc;
        s->lpt_steps_ready = false;
        s->lpt_next *= 8;
      }
      if ((rc = s->launch_fused_step(0, r.tau, K))) return rc;
      if (s->lpt_next > 0 && s->steps_d.p && !lpt_sorted_now) {
        if (s->lpt_iters + K >= s->lpt_next) {
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
  r.from_batch = s->bt.len > 0;
  // the next iteration's y-solve may follow this iteration's last kernel at once (fetch_out, solve_next): the whole solve is on the
  // device and belongs to the engine (not to a closed block's kernel), sigma does not change in this iteration's step 5, nothing of a
  // batch is pending, and the per-class event timers (profile = 1) are off -- they are collected at the wait, before that solve ends
  r.solve_next_ok = s->sw.solve_next != 0 && !s->accel_on() && !s->infeas_on() && !s->gap_on() && s->dev_solve && !r.from_batch && !r.sig_may_change && !(s->fuse && s->closed.active) && s->profile != 1;
  return CUADMM_OK;
}

// developer aid (option debug_eig + CUADMM_DEBUG_EIG=<dir>): dump the projection input when a block hits the QL cap
static void dump_failed_projection(Solver* s, int iter, const char* dir) {
  int f = s->plan.fail_count(s->st);
  if (f == s->eig_fail_total) return;
  fprintf(stderr, "[cuadmm debug] iter %d: QL cap hits %d -> %d\n", iter, s->eig_fail_total, f);
  std::vector<double> h((size_t)s->L);
  if (staged_d2h(h.data(), s->Xb.p, sizeof(double) * (size_t)s->L, s->st) == CUADMM_OK) {
    char fn[256];
    snprintf(fn, sizeof fn, "%s/xb_fail_iter%d.bin", dir, iter);
    if (FILE* fp = fopen(fn, "wb")) { fwrite(h.data(), sizeof(double), (size_t)s->L, fp); fclose(fp); }
  }
  s->eig_fail_total = f;
}

// y up, then Rd1 / Xb and the projection: fused with the post step that follows it, or kernel by kernel
static int run_projection(Solver* s, const SolveRun& r) {
  int rc;
  if ((rc = s->upload_y())) return rc;
  if (s->fuse) return s->launch_fused_step((r.iter < r.switch_admm || r.snapshot) ? 1 : 0, r.tau);
  if ((rc = s->launch_aty(true))) return rc;
  s->plan.rank_active = s->eig_rank > 0 && (r.iter >= s->eig_rank_begin_iter || s->maxfeas < s->eig_rank_maxfeas);   // duo_solver.cu:844
  if ((rc = s->launch_project())) return rc;
  const char* const debug_eig_dir = s->sw.debug_eig ? getenv("CUADMM_DEBUG_EIG") : nullptr;
  if (debug_eig_dir) dump_failed_projection(s, r.iter, debug_eig_dir);
  return CUADMM_OK;
}

// sGS half step: S^{k+1}, second solve with it, Rd1 from the new y (solver.cu:693-729)
static int run_sgs_half(Solver* s, const SolveRun& r) {
  int rc;
  const int m = s->m;
  if (!s->fuse && (rc = s->launch_post_mode(1, r.tau))) return rc;     // fused: done with the projection
  if ((rc = s->launch_spmv(false, true, s->fuse))) return rc;
  if ((rc = s->fetch_out((size_t)m + 2, (size_t)m))) return rc;
  if ((rc = s->host_solve())) return rc;
  if ((rc = s->upload_y())) return rc;
  if (s->At_long.nlong == 0 && s->sw.aty_post2) {   // one pass, Rd1 not stored (vec_kernels.hip)
    s->prof_begin(K_POST);
    rc = launch_aty_post2(s->L, s->At_rp.p, s->At_ci.p, s->At_v.p, s->y_d.p, s->C.p, s->S.p, s->X.p, r.tau * s->sig, s->partials.p,
                          s->out_w + (size_t)m, s->st);
    s->prof_end(K_POST, 40.0 * (double)s->L);
    if (rc) return rc;
  } else {
    if ((rc = s->launch_aty(false))) return rc;
    if ((rc = s->launch_post_mode(2, r.tau))) return rc;
  }
  if ((rc = s->launch_spmv(true, false))) return rc;
  return s->fetch_out(0, (size_t)m + 2, r.solve_next_ok);   // [A*X | sums]; A*(S-C) unchanged since the half step
}

// ADMM: the S and X updates behind the projection, around the snapshot of the best iterate when this iteration takes one
static int run_admm_post(Solver* s, const SolveRun& r) {
  int rc;
  const int m = s->m;
  const long long L = s->L;
  if (r.snapshot) {
    if (!s->X_best.p && L > 0) { if ((rc = s->X_best.alloc(L)) || (rc = s->S_best.alloc(L))) return rc; }
    if (!s->fuse && (rc = s->launch_post_mode(1, r.tau))) return rc;
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
    if ((rc = s->launch_post_mode(2, r.tau))) return rc;
  } else if (!s->fuse) {
    if ((rc = s->launch_post_mode(0, r.tau))) return rc;
  }
  if ((rc = s->launch_spmv(true, true, s->fuse && !r.snapshot))) return rc;
  return s->fetch_out(0, 2 * (size_t)m + 2, r.solve_next_ok);
}

// ---- Step 5 (solver.cu:764-799): the four scalars from where this iteration left them, the stopping test's state, sigma, the info arrays
static int take_scalars(Solver* s, SolveRun& r) {
  int rc;
  const int m = s->m;
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
  double v[4] = {nr, bty, s->h_out.p[(size_t)m], s->h_out.p[(size_t)m + 1]};
  if (r.from_batch) {
    for (int q = 0; q < 4; ++q) v[q] = s->bt.h.p[4 * (size_t)s->bt.pos + q];
    if (++s->bt.pos == s->bt.len) s->bt.len = s->bt.pos = 0;
  } else if (s->dev_scalars || s->dev_solve) { for (int q = 0; q < 4; ++q) v[q] = s->h_scal.p[q]; }   // formed (and summed over ranks) on the device
  else if ((rc = s->allreduce_scalars(v, 4))) return rc;
  nr = v[0]; bty = v[1]; s->h_out.p[(size_t)m] = v[2]; s->h_out.p[(size_t)m + 1] = v[3];
  // a lost row exchange of the four-workgroups-per-row tail kernel leaves NaN in y and with it in these sums: stop NOW (not at
  // max_iter), report once, and leave the handle on the two-GEMV path (TailSolve::take_failure)
  if (s->tail.d_fail && !(std::fabs(nr) <= 1.7976931348623157e308 && std::fabs(bty) <= 1.7976931348623157e308) && (rc = tail_failure(s, r.iter))) return rc;
  s->set_residual_scalars(nr, bty);
  s->feasratio = s->ratioconst * s->errRp / s->errRd;
  if (s->feasratio < 1) s->prim_win += 1; else s->dual_win += 1;
  if (r.sig_may_change) {
    if (s->prim_win > 1.2 * s->dual_win) { s->prim_win = 0; s->sig = std::min(s->sigmax, s->sig * r.sigscale); }
    else if (s->dual_win > 1.2 * s->prim_win) { s->dual_win = 0; s->sig = std::max(s->sigmin, s->sig / r.sigscale); }
  }
  s->prof_host(K_HOST, wall_s() - t0);
  s->info[CUADMM_INFO_POBJ].push_back(s->pobj); s->info[CUADMM_INFO_DOBJ].push_back(s->dobj);
  s->info[CUADMM_INFO_ERRRP].push_back(s->errRp); s->info[CUADMM_INFO_ERRRD].push_back(s->errRd);
  s->info[CUADMM_INFO_RELGAP].push_back(s->relgap); s->info[CUADMM_INFO_SIG].push_back(s->sig);
  s->info[CUADMM_INFO_BSCALE].push_back(s->bscale); s->info[CUADMM_INFO_CSCALE].push_back(s->Cscale);
  s->info_iter_num++;
  return CUADMM_OK;
}

// longest block first (PsdPlan::reorder_by_steps): at iterations 3, 24, 192, ... of this solve the stream is idle here
static int lpt_reorder(Solver* s) {
  int rc;
  if (!s->fuse || s->lpt_next <= 0) return CUADMM_OK;
  ++s->lpt_iters;
  if (s->lpt_iters >= s->lpt_next && s->bt.len == 0 && s->steps_d.p && !s->can_batch()) {
    s->steps_h.resize(s->steps_d.n);
    if ((rc = staged_d2h(s->steps_h.data(), s->steps_d.p, sizeof(int) * s->steps_d.n, s->st))) return rc;
    if ((rc = s->plan.reorder_by_steps(s->steps_h.data(), s->st))) return rc;
    s->lpt_next *= 8;
  }
  return CUADMM_OK;
}

// unscale (solver.cu:814-816) -- deferred until somebody reads or replaces X, y, S (materialise): a following
// solve(if_first = false) continues from the scaled state.  With owned constraints over several ranks the y gather is a
// collective, so there it happens here, where every rank is.
static int solve_end(Solver* s) {
  int rc;
  s->pending_unscale = true;
  if (s->lazy_unscale == 0 || (s->local_mode && s->comm_world > 1)) { if ((rc = s->materialise())) return rc; }
  if (s->tail.k > 0 && (rc = tail_failure(s, 0))) return rc;
  s->eig_fail_total = s->plan.fail_count(s->st);
  if (s->eig_fail_total > 0) {
    set_error("solve: %d block projections hit the QL sweep cap", s->eig_fail_total);
    return CUADMM_ERR_EIG;
  }
  return CUADMM_OK;
}

extern "C" {

int cuadmm_solve(cuadmm_solver* s, int max_iter, double stop_tol, int sig_update_threshold, int sig_update_stage_1,
                 int sig_update_stage_2, int switch_admm, double sigscale, int if_first) {
  // (the argument checks precede the group forward: the leader's error is raised on the caller's thread, before any rank starts)
  if (!s || !s->initialised) { set_error("solve: solver not initialised"); return CUADMM_ERR_INVALID; }
  if (s->factor_bad) { set_error("solve: the last cuadmm_update_A could not factor the new A A^T; the solver needs a successful cuadmm_update_A first"); return CUADMM_ERR_FACTOR; }
  if (sig_update_stage_1 <= 0 || sig_update_stage_2 <= 0) { set_error("solve: sig_update stages must be positive"); return CUADMM_ERR_INVALID; }
  if (s->group && !s->in_group_call)      // the leader of an in-process group (duo_group.hip): every rank solves, on its own host thread
    return group_forward(s, [&](cuadmm_solver* q) {
      return cuadmm_solve(q, max_iter, stop_tol, sig_update_threshold, sig_update_stage_1, sig_update_stage_2, switch_admm, sigscale, if_first);
    });
  SolveRun r{max_iter, stop_tol, sig_update_threshold, sig_update_stage_1, sig_update_stage_2, switch_admm, sigscale, if_first};
  int rc;
  if ((rc = solve_begin(s, r))) return rc;
  for (r.iter = 1; r.iter <= max_iter + 1; ++r.iter) {
    if ((rc = stop_test(s, r))) return rc;                               // Step 0
    // ---- Step 1 (solver.cu:478-500): y = (AA^T)^-1 (Rp/sig - A(S-C)); with closed blocks the fused projection of this
    // iteration solves it (not on the last pass through the loop, which stops before the projection)
    if (s->y_early) s->y_early = false;       // enqueued at the end of the previous iteration (fetch_out, solve_next)
    else if (s->solve_status == 5) {}         // the bound was formed at the y the solve returns: no further y-solve behind the verdict
    else if (s->bt.len == 0 && (rc = s->host_solve(s->fuse && !r.breakyes))) return rc;
    if (r.breakyes) {
      if ((rc = restore_best(s, r))) return rc;
      break;
    }
    if ((rc = plan_iteration(s, r)) || (rc = batch_begin(s, r))) return rc;       // Step 2: the decisions, then the device
    if (!r.from_batch) {                      // (a batch's iterations ran in its launch: their scalars wait in bt.h)
      if ((rc = run_projection(s, r))) return rc;
      if ((rc = r.iter < switch_admm ? run_sgs_half(s, r) : run_admm_post(s, r))) return rc;
    }
    const double sig_of_iter = s->sig;
    if ((rc = take_scalars(s, r)) || (rc = lpt_reorder(s))) return rc;            // Step 5
    // ---- acceleration: behind the iteration, on every path (the scalars above are those of the plain iterate f_k)
    if (s->accel_on() && (rc = s->accel_step(r.iter, max_iter, stop_tol, switch_admm, r.tau, s->sig != sig_of_iter, r.sig_may_change_at(r.iter + 1)))) return rc;
    // ---- infeasibility check: on the state at the end of the iteration, after the sigma update
    if (s->infeas_on() && r.iter % s->inf.period == 0 && (rc = s->infeas_step(r.iter, stop_tol))) return rc;
    // ---- certified-gap check: the lower bound at this iteration's y against this iteration's pobj
    if (s->gap_on() && r.iter % s->lb.period == 0 && (rc = s->lb_step(r.iter, stop_tol))) return rc;
  }
  return solve_end(s);
}

int cuadmm_duo_solve(cuadmm_solver* s, int max_iter, double stop_tol, int sig_update_threshold, int sig_update_stage_1,
                     int sig_update_stage_2, int switch_admm, double sigscale, int if_first) {
  return cuadmm_solve(s, max_iter, stop_tol, sig_update_threshold, sig_update_stage_1, sig_update_stage_2, switch_admm, sigscale, if_first);
}

}  // extern "C"
