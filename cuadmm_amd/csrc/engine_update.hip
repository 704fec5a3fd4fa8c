// What changes a solver between two solves: cuadmm_set_XyS, cuadmm_update_bC, cuadmm_update_A.  They share init's normalisation helpers and
// stages (engine_state.h), not the loop.  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "engine_state.h"

using namespace cuadmm;

extern "C" {

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

// X or S from per-block factors, X_k = L_k L_k' (lowrank_apply.h): cuadmm_set_XyS for that one vector without the vector -- the factors are
// staged (one copy of the factor buffer) and one kernel pass writes svec(L_k L_k') into the resident iterate.  Every check runs before
// anything changes, materialise() included.
int cuadmm_set_lowrank(cuadmm_solver* s, int which, const double* L, const int* ranks, int rmax, double sig, double out4[4]) {
  if (!s || !s->initialised) { set_error("set_lowrank: not initialised"); return CUADMM_ERR_INVALID; }
  if (which < 0 || which > 1) { set_error("set_lowrank: which = %d (0: X, 1: S)", which); return CUADMM_ERR_INVALID; }
  if (rmax < 1 || rmax > kMaxBlockSize) { set_error("set_lowrank: rmax = %d, allowed are 1 to %d", rmax, kMaxBlockSize); return CUADMM_ERR_INVALID; }
  if (!ranks) { set_error("set_lowrank: ranks is null"); return CUADMM_ERR_INVALID; }
  if (s->world > 1 || s->comm_world > 1 || s->local_mode || s->group || s->in_group_call) {
    set_error("set_lowrank: works on one rank (world = %d%s)", std::max(s->world, s->comm_world), s->group ? ", in-process group" : "");
    return CUADMM_ERR_INVALID;
  }
  const int nb = (int)s->blk_local.size();
  double blocks = 0, rank_sum = 0;
  int rc = check_factors("set_lowrank", nb, s->blk_local.data(), ranks, rmax, "L", L, nullptr, nullptr, &blocks, &rank_sum);
  if (rc || (rc = check_device(s->device))) return rc;
  // the layout, the plan and the staged factors: buffers of the low-rank calls' own
  if (!s->btasks.built && (rc = s->btasks.build(s->blk_local.data(), nb, nullptr))) return rc;
  if ((rc = s->fl.prepare(s->blk_local.data(), nb, rmax)) || (rc = s->lo.prepare(s->fl, s->blk_local.data())) || (rc = s->fl.stage(s->lo.Lbuf, L)) ||
      (rc = s->fl.stage_ranks(ranks)))
    return rc;
  const double bytes = L ? 8.0 * (double)s->fl.count() : 0.0;
  // --- from here on the solver changes
  if ((rc = s->materialise())) return rc;       // the vectors NOT replaced must be in the caller's units too
  CUADMM_HIP_TRY(hipEventRecord(s->lo.ev[0], s->st));
  if ((rc = s->lo.run(s->fl, s->lo.Lbuf.p, s->btasks.off.p, s->btasks.blk.p, which == 0 ? s->X.p : s->S.p, s->st))) return rc;
  CUADMM_HIP_TRY(hipEventRecord(s->lo.ev[1], s->st));
  CUADMM_HIP_TRY(hipStreamSynchronize(s->st));
  if (sig > 0) s->sig = sig;
  s->infeas_reset();                            // snapshots and status describe another iterate
  s->lb_reset();
  if (out4) { out4[0] = blocks; out4[1] = rank_sum; out4[2] = event_ms(s->lo.ev[0], s->lo.ev[1]); out4[3] = bytes; }
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
  if (timed) for (auto& e : s->upa.ev) if (!e && (rc = e.create())) return rc;
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

}  // extern "C"
