// What the reports on a point own beside the iteration's state, and what the op hooks build on their own: the auxiliary projector, the
// per-block task lists, the plan of cuadmm_lambda_min, and for the low-rank calls (cuadmm_lowrank, cuadmm_set_lowrank,
// cuadmm_block_multiply, cuadmm_lowrank_grad, cuadmm_lowrank_line, cuadmm_lowrank_refine) the one factor layout on the device, each kernel's task list and
// buffers, and the host helpers the calls share.  Nothing here is read by the iteration.
#pragma once
#include <algorithm>
#include <cmath>

#include "dev_buf.h"
#include "factor_layout.h"
#include "psd_plan.h"
#include "block_reduce.h"
#include "lambda_min.h"
#include "lowrank.h"
#include "lowrank_apply.h"
#include "block_mult.h"
#include "lowrank_grad.h"
#include "lowrank_line.h"
#include "lowrank_refine.h"

struct cuadmm_solver;

namespace cuadmm {

// The auxiliary projector of the infeasibility check and the lower bound ("Infeasibility certificates"): a plan beside the
// iteration's, an svec-length input and output vector, b on the device where the engine keeps none there, a pair of events.  The two
// users never run inside one another and the plan carries no result from one projection to the next, so one object serves both.
struct AuxProj {
  PsdPlan* plan = nullptr;           // built at the first projection: the solver's psd_* options, the full projection
  DevBuf<double> in, out, bcopy;
  double plan_bytes = 0;
  DevEvent ev[2];
  bool projected = false;            // inside the open bracket
  int ensure(cuadmm_solver& s);      // vectors and events on first use; b, which may have changed, on every call
  const double* b_dev(const cuadmm_solver& s) const;      // (engine_state.h, behind the solver's definition)
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
  ~AuxProj() { delete plan; }
};

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
};

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
};

static_assert(kFactorMaxBlock == kMaxBlockSize, "factor_layout.h refuses what the plans refuse");

// Rank and low-rank factor per block (cuadmm_lowrank, cuadmm_op_block_lowrank; lowrank.h, DESIGN.md "Low-rank factors"): the size
// classes' block lists, the offsets of the blocks' factors (factor_layout.h) and pivots for the rmax of the last call, the factor, pivot
// and result buffers (they grow with rmax and are kept), a pair of events.  The kernel writes the factors, so they are its own and not the
// callers' (FactorLayoutDev).  The offsets and sizes per block are the task lists' (btasks).  Nothing here is read by the iteration.
struct LrPlan {
  LrClass cls[kLrClasses];
  DevBuf<int> list[kLrClasses], piv;
  DevBuf<long long> loff_d, poff_d;
  DevBuf<double> Lbuf, out;
  std::vector<long long> loff, poff;      // of rmax_now, nb + 1 entries each
  int nb = 0, rmax_now = 0;
  DevEvent ev[2];
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
      for (auto& e : ev) if ((rc = e.create())) return rc;
    }
    rmax_now = 0;                           // (until the offsets on the device are this rmax's)
    if ((rc = loff_d.upload(loff.data(), loff.size())) || (rc = poff_d.upload(poff.data(), poff.size()))) return rc;
    if ((rc = Lbuf.grow((size_t)loff.back() + 1)) || (rc = piv.grow((size_t)poff.back() + 1))) return rc;      // (+ 1: never empty)
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
  // (may be null): loff.back() doubles; piv_out (may be null): as many ints, block k's pivots at loff[k], -1 elsewhere.
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
};

// The layout of the callers' factors on the device (factor_layout.h), one per solver for cuadmm_set_lowrank, cuadmm_block_multiply,
// cuadmm_lowrank_grad and cuadmm_lowrank_line, and one per call of an op hook: the offsets of the rmax they were last asked for, here
// and on the device, and the device copy of the ranks.  Every call prepares it for its own rmax first, so whatever it launches reads
// offsets and ranks of one rmax; the buffers that hold factors are the users' and grow to count() + 1 (never empty).
struct FactorLayoutDev {
  std::vector<long long> loff;              // of rmax_now, nb + 1 entries
  DevBuf<long long> loff_d;
  DevBuf<int> ranks_d;
  int nb = 0, rmax_now = 0;
  int prepare(const int* blk_h, int nblk, int rmax) {
    if (ranks_d.p && rmax == rmax_now) return CUADMM_OK;
    int rc = factor_offsets("factor_layout", nblk, blk_h, rmax, &loff);
    if (rc) { rmax_now = 0; return rc; }
    if (!ranks_d.p && (rc = loff_d.alloc((size_t)nblk + 1))) return rc;
    rmax_now = 0;                           // (until the offsets on the device are this rmax's)
    if ((rc = loff_d.upload(loff.data(), loff.size()))) return rc;
    nb = nblk;
    rmax_now = rmax;
    return ranks_d.p ? CUADMM_OK : ranks_d.alloc((size_t)nblk + 1);      // last: marks the set as complete
  }
  size_t count() const { return (size_t)loff.back(); }
  int stage_ranks(const int* ranks) { return ranks_d.upload(ranks, (size_t)nb); }
  // a factor buffer whole, in one copy (null: nothing, every rank is 0)
  int stage(DevBuf<double>& buf, const double* host) const { return host ? buf.upload(host, count()) : CUADMM_OK; }
  double bytes() const { return 8.0 * (double)loff_d.n + 4.0 * (double)ranks_d.n; }
};

// dst <- the factors src in the units a vector of unit ux lies in: fl(src[e] * root), root = fl(1 / sqrt(ux)), in the columns that are read
// and + 0.0 in the others.  cuadmm_lowrank_grad's L and cuadmm_lowrank_line's L and D go through here: the same L gives the same bits.
inline void scale_factors(const FactorLayoutDev& fl, const int* blk_h, const int* ranks, const double* src, double ux, std::vector<double>& dst) {
  const double root = 1 / std::sqrt(ux);
  dst.assign(fl.count(), 0.0);
  for (int k = 0; k < fl.nb; ++k)
    for (size_t e = (size_t)fl.loff[k], end = e + (blk_h[k] > 0 ? (size_t)blk_h[k] * (size_t)ranks[k] : 0); e < end; ++e) dst[e] = src[e] * root;
}
// out[perm[i]] <- h[i]: an m-vector from the factor's order to the caller's (out may be null)
inline void unpermute(const std::vector<int>& perm, int m, const double* h, double* out) {
  for (int i = 0; out && i < m; ++i) out[perm[i]] = h[i];
}
// a kernel's kBrSlots slot partials added in slot order from 0.0
inline double slot_sum(const double* part) {
  double s = 0;
  for (int j = 0; j < kBrSlots; ++j) s = s + part[j];
  return s;
}

// Start from low-rank factors (cuadmm_set_lowrank, cuadmm_op_block_outer; lowrank_apply.h, DESIGN.md "Starting from low-rank factors"):
// the wavefront task list, built once (it depends on the block sizes alone), a device factor buffer that grows with the layout and is
// kept, a pair of events.  The offsets and sizes per block are the task lists' (btasks).  Nothing here is read by the iteration.
struct LoPlan {
  std::vector<LoTask> tasks;
  DevBuf<LoTask> tasks_d;
  DevBuf<double> Lbuf;
  DevEvent ev[2];
  int prepare(const FactorLayoutDev& fl, const int* blk_h, int split_from = kLoSplitFrom) {
    int rc;
    if (!ev[1]) {
      if ((rc = lo_build_tasks(fl.nb, blk_h, fl.rmax_now, split_from, &tasks, nullptr)) || (rc = tasks_d.from(tasks, 1))) return rc;      // (+ 1: never empty)
      for (auto& e : ev) if ((rc = e.create())) return rc;
    }
    return Lbuf.grow(fl.count() + 1);
  }
  // v (device) <- svec(L_k L_k') on every PSD block from the device factors L, one launch
  int run(const FactorLayoutDev& fl, const double* L, const long long* off_d, const int* blk_d, double* v, hipStream_t st) {
    return launch_block_outer((int)tasks.size(), tasks_d.p, L, fl.loff_d.p, fl.ranks_d.p, off_d, blk_d, v, st);
  }
  double bytes() const { return 8.0 * (double)Lbuf.n + (double)sizeof(LoTask) * (double)tasks_d.n; }
};

// Blocks times factors (cuadmm_block_multiply, cuadmm_op_block_mult; block_mult.h, DESIGN.md "Blocks times factors"): the wavefront
// task list, built once (it depends on the block sizes alone), the device V and W (they grow with the layout and are kept), the y of
// which = 2, a pair of events.  V travels whole in one staged copy and W comes back whole, padding columns included; both copies lie
// outside the timed interval.  The offsets and sizes per block are the task lists' (btasks).  Nothing here is read by the iteration.
struct BmPlan {
  std::vector<BmTask> tasks;
  DevBuf<BmTask> tasks_d;
  DevBuf<double> Vbuf, Wbuf, ybuf;
  DevEvent ev[2];
  long long calls = 0;
  int prepare(const FactorLayoutDev& fl, const int* blk_h) {
    int rc;
    if (!ev[1]) {
      if ((rc = bm_build_tasks(fl.nb, blk_h, fl.rmax_now, &tasks, nullptr)) || (rc = tasks_d.from(tasks, 1))) return rc;      // (+ 1: never empty)
      for (auto& e : ev) if ((rc = e.create())) return rc;
    }
    if ((rc = Vbuf.grow(fl.count() + 1))) return rc;
    return Wbuf.grow(fl.count() + 1);
  }
  // Wbuf (device) <- sign * M_k V_k on every PSD block of v, one launch
  int run(const FactorLayoutDev& fl, const double* v, double sign, const long long* off_d, const int* blk_d, hipStream_t st) {
    return launch_block_mult((int)tasks.size(), tasks_d.p, v, sign, Vbuf.p, Wbuf.p, fl.loff_d.p, fl.ranks_d.p, off_d, blk_d, st);
  }
  // W_out (fl.count() doubles, host) behind a drained stream: the kernel's entries times `unit`, + 0.0 in the columns >= ranks[k]
  int fetch(const FactorLayoutDev& fl, const int* blk_h, const int* ranks, double unit, double* W_out) {
    int rc;
    if (fl.count() > 0 && (rc = staged_d2h(W_out, Wbuf.p, sizeof(double) * fl.count()))) return rc;
    for (int k = 0; k < fl.nb; ++k) {
      if (blk_h[k] <= 0) continue;
      double* const w = W_out + fl.loff[k];
      const size_t used = (size_t)blk_h[k] * (size_t)ranks[k];
      for (size_t e = 0; unit != 1.0 && e < used; ++e) w[e] *= unit;
      std::fill(w + used, W_out + fl.loff[k + 1], 0.0);
    }
    return CUADMM_OK;
  }
  double bytes() const { return 8.0 * (double)(Vbuf.n + Wbuf.n + ybuf.n + tasks_d.n); }
};

// Value and gradient at factors (cuadmm_lowrank_grad; lowrank_grad.h, DESIGN.md "Value and gradient at factors"): the svec vector x is
// assembled in (a device copy of X with svec(L_k L_k') over its PSD blocks), the m-vectors of the multiplier pass (y, A x, ytilde, r; the
// column norms where the engine keeps none on the device), the slot partials, the per-block sums and a pair of events.  The factors are
// the block product's V (BmPlan) and the outer product (LoPlan's task list) reads them there where x is in the caller's units, else from
// LoPlan's buffer; both launches read the solver's one FactorLayoutDev.  The products go to BmPlan's W and A'ytilde - C to the auxiliary
// projector's input vector.  Nothing here is read by the iteration.
struct LgPlan {
  DevBuf<double> xv, ybuf, ax, ytilde, r, normA, part, sums, cpart;
  std::vector<double> h_stage, h_back, h_G;      // host scratch kept between calls: the scaled factors, what comes back, G where the caller wants none
  DevEvent ev[2];
  int prepare(long long L, int m, int nb, int nchunk, bool own_normA) {
    if (sums.p) return CUADMM_OK;
    int rc;
    const size_t mm = (size_t)std::max(m, 1);
    if ((rc = xv.alloc((size_t)L)) || (rc = ybuf.alloc(mm)) || (rc = ax.alloc(mm)) || (rc = ytilde.alloc(mm)) || (rc = r.alloc(mm)) ||
        (own_normA && (rc = normA.alloc(mm))) || (rc = part.alloc(2 * (size_t)kBrSlots)) || (rc = cpart.alloc(kLgSums * (size_t)std::max(nchunk, 1))))
      return rc;
    for (auto& e : ev) if ((rc = e.create())) return rc;
    return sums.alloc(kLgSums * (size_t)std::max(nb, 1));      // last: marks the set as complete
  }
  double bytes() const { return 8.0 * (double)(xv.n + ybuf.n + ax.n + ytilde.n + r.n + normA.n + part.n + sums.n + cpart.n); }
};

// The quartic along a line in factor space (cuadmm_lowrank_line; lowrank_line.h, DESIGN.md "Line search along factor steps"): the three
// svec vectors x0 (a device copy of X with svec(L_k L_k') over its PSD blocks), x1 and x2 (zeroed once, here: the kernel writes their PSD
// slots only, and always all of them, so the unconstrained slices stay zero), the device copy of D (it grows with the layout; L travels
// in LoPlan's buffer, whose task list the launch walks with the solver's FactorLayoutDev), the m-vectors of the streaming pass (y, the
// three A x, r0, p, q; the column norms where the engine keeps none on the device), the slot partials, the per-block sums and a pair of
// events.  Nothing here is read by the iteration.
struct LlPlan {
  DevBuf<double> x0, x1, x2, Dbuf, ybuf, ax0, ax1, ax2, r0, p, q, normA, part, sums, cpart;
  std::vector<double> h_L, h_D, h_back;          // host scratch kept between calls: the scaled factors, what comes back
  DevEvent ev[2];
  int prepare(long long L, int m, int nb, int nchunk, bool own_normA, hipStream_t st) {
    if (sums.p) return CUADMM_OK;
    int rc;
    const size_t mm = (size_t)std::max(m, 1);
    if ((rc = x0.alloc((size_t)L)) || (rc = x1.alloc((size_t)L)) || (rc = x2.alloc((size_t)L)) || (rc = ybuf.alloc(mm)) || (rc = ax0.alloc(mm)) ||
        (rc = ax1.alloc(mm)) || (rc = ax2.alloc(mm)) || (rc = r0.alloc(mm)) || (rc = p.alloc(mm)) || (rc = q.alloc(mm)) || (own_normA && (rc = normA.alloc(mm))) ||
        (rc = part.alloc(kLlParts * (size_t)kBrSlots)) || (rc = cpart.alloc(kLlSums * (size_t)std::max(nchunk, 1))))
      return rc;
    CUADMM_HIP_TRY(hipMemsetAsync(x1.p, 0, sizeof(double) * (size_t)L, st));
    CUADMM_HIP_TRY(hipMemsetAsync(x2.p, 0, sizeof(double) * (size_t)L, st));
    for (auto& e : ev) if ((rc = e.create())) return rc;
    return sums.alloc(kLlSums * (size_t)std::max(nb, 1));      // last: marks the set as complete
  }
  double bytes() const {
    return 8.0 * (double)(x0.n + x1.n + x2.n + Dbuf.n + ybuf.n + ax0.n + ax1.n + ax2.n + r0.n + p.n + q.n + normA.n + part.n + sums.n + cpart.n);
  }
};

// Conjugate gradients over the factors (cuadmm_lowrank_refine; lowrank_refine.h, DESIGN.md "Refinement over factors"): the two factor-sized
// device buffers the loop adds -- the direction in the caller's units and the previous gradient; L lives in BmPlan's V (caller's units) and
// LoPlan's buffer (the units X lies in), the scaled direction in LlPlan's D, the gradient in BmPlan's W -- the slot partials of the three
// sums, the host scratch kept between calls and the events: one pair around the loop and two pairs the steps take in turn, so that a
// step's interval is read behind the next step's first synchronisation.  Nothing here is read by the iteration.
struct RfPlan {
  DevBuf<double> D, Gold, part;
  std::vector<double> h_L, h_part;
  DevEvent ev[6];
  long long calls = 0;
  int prepare(const FactorLayoutDev& fl) {
    int rc;
    if (!part.p) {
      for (auto& e : ev) if ((rc = e.create())) return rc;
    }
    if ((rc = D.grow(fl.count() + 1)) || (rc = Gold.grow(fl.count() + 1))) return rc;
    return part.p ? CUADMM_OK : part.alloc(kRfParts * (size_t)kBrSlots);      // last: marks the set as complete
  }
  double bytes() const { return 8.0 * (double)(D.n + Gold.n + part.n); }
};

}  // namespace cuadmm
