"""cuadmm_evaluate on the GPU (include/cuadmm_amd.h; DESIGN.md, "Evaluation of a point"; csrc/evaluate.hip; csrc/engine_reports.hip: ev_run):
the per-block statistics kernel against numpy, the report against the longdouble twin (tests/_evaluate_twin.py) at a known optimum,
at known violations, at the engine's own iterate and in the engine's other plans, its absence of side effects, the refusals and the
command line.

Tolerances (U = 2^-53), all from the twin's own numbers:
  a sum of the kernel            len_k U sum |terms| against the longdouble sum: holds for every summation order
  norms                          64 U times the norm; inner products: 64 U sum |terms| (the twin's absolute sums)
  vX_k, vS_k                     2e-12 sqrt(len_k) ||._k||, twice the projection kernels' contract (nu_tolerance of the lower bound's tests)
  ||A X - b||, ||Rd_k||          the 2-norm of the entrywise bound (row or column length + 8) U (|A||X| + |b|), resp.
                                 (|C| + |A|'|y| + |S|) (form_error of the lower bound's tests), plus 64 U times the norm as there
  vX, vS, ||Rd||                 the 2-norm of the per-block tolerances (| ||a|| - ||b|| | <= ||a - b||), plus 64 U times the norm
  err1 .. err4                   the numerator's tolerance over the denominator, plus 64 U |err|
  err5, err6                     (tol pobj + tol dobj [+ tol <X,S>]) / den for the numerator and as much for the denominator
                                 (|err| <= 1), plus 64 U |err|
"""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd import synthetic
from tests._evaluate_twin import KEYS, evaluate
from tests._infeas_twin import Fixture, smat, svec
from tests._lower_bound_twin import blk_lens, make_opt_fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
U = 2.0 ** -53
LD = np.longdouble
INFO = ("pobj", "dobj", "errRp", "errRd", "relgap", "sig", "bscale", "Cscale")
BLK_A, M_A = [3, 20, 70, -2, 130], 40                     # register, one-wavefront, LDS and cluster classes, a free block
BLK_B, M_B = [1] * 40 + [2, 5, 8, -3, 33], 30             # odd offsets
_fx = {}


def fixture(name):
    if name not in _fx:
        _fx[name] = make_opt_fixture(BLK_A, M_A, 1) if name == "A" else make_opt_fixture(BLK_B, M_B, 1)
    return _fx[name]


def amd(fx):
    r, c, v = fx.coo()
    bi, ci = np.nonzero(fx.b)[0], np.nonzero(fx.C)[0]
    return cuadmm_amd.Problem.from_coo(fx.blk, fx.m, r, c, v, bi, fx.b[bi], ci, fx.C[ci])


def solver(fx, options=None, **kw):
    s = cuadmm_amd.SDPSolver(verbose=False, options=options, **kw)
    s.init_problem(amd(fx))
    return s


def offsets(blk):
    return np.concatenate([[0], np.cumsum(blk_lens(blk))])


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------
OP_LISTS = {
    "mixed": [1] * 37 + [2, 3, 5, 8] + [-1, -7] + [9, 31, 64, 65] + [-130] + [200],        # 200: 20 100 slots, three chunks
    "n600": [600],                                                                          # 180 300 slots: 23 chunks
    "many3": [3] * 20000,
}


def _op(vecs, blk, offs, offset):
    lib = cuadmm_amd.load()
    blk = np.asarray(blk, np.int32)
    v = [a.copy() for a in vecs]
    sums = np.zeros(6 * blk.size)
    rc = lib.cuadmm_op_ev_block_stats(v[0].size, P(v[0]), P(v[1]), P(v[2]), P(v[3]), P(v[4]), blk.size, P(blk), P(offs), offset, P(sums))
    assert rc == 0, lib.cuadmm_last_error()
    return v, sums.reshape(-1, 6)


def _terms(X, S, PX, PS, R1, free):
    """the six term vectors of one block: the differences and Rd1 + S as float64 forms them, the products exact (longdouble)"""
    dx = np.zeros_like(X) if free else PX - X
    ds = S if free else PS - S
    rd = R1 + S
    l = lambda a: a.astype(LD)
    return [l(X) * l(X), l(dx) * l(dx), l(S) * l(S), l(ds) * l(ds), l(X) * l(S), l(rd) * l(rd)]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", list(OP_LISTS))
def test_block_stats_kernel(name, offset):
    blk = OP_LISTS[name]
    rng = np.random.default_rng(len(blk) + offset)
    lens = blk_lens(blk)
    gaps = rng.integers(0, 4, size=len(blk))                     # arbitrary offsets: up to three slots between two blocks, NaN in them
    offs = (np.concatenate([[0], np.cumsum(lens + gaps)[:-1]]) + 1).astype(np.int64)
    n = int(offs[-1] + lens[-1] + 2)
    vecs = [np.full(n, np.nan) for _ in range(5)]
    for o, ln in zip(offs, lens):
        for v in vecs:
            v[o:o + ln] = rng.standard_normal(ln) * 10.0 ** rng.integers(-3, 4)
    back, sums = _op(vecs, blk, offs, offset)
    for a, b in zip(vecs, back):
        assert np.array_equal(a, b, equal_nan=True)              # nothing is written to the vectors
    worst = 0.0
    for k, (o, ln) in enumerate(zip(offs, lens)):
        for q, t in enumerate(_terms(*[v[o:o + ln] for v in vecs], blk[k] < 0)):
            want, bound = float(np.sum(t)), float(ln * U * np.sum(np.abs(t)))
            worst = max(worst, abs(sums[k, q] - want) / bound if bound > 0 else 0.0)
            assert abs(sums[k, q] - want) <= bound, (k, blk[k], q, sums[k, q], want)
        if blk[k] < 0:
            assert sums[k, 1] == 0.0 and sums[k, 3] == sums[k, 2]
    print("%s offset %d: worst sum error / bound %.3f" % (name, offset, worst))
    _, sums2 = _op(vecs, blk, offs, offset)
    assert np.array_equal(sums, sums2)                           # bit-identical from run to run


def test_block_stats_kernel_consecutive_blocks_and_validation():
    """offs = NULL: one block behind the other, as the engine lays them out; a block outside the vectors is refused before a launch"""
    blk = OP_LISTS["mixed"]
    lens = blk_lens(blk)
    rng = np.random.default_rng(7)
    vecs = [rng.standard_normal(int(lens.sum())) for _ in range(5)]
    off = offsets(blk)
    for offset in (0, 1):
        _, sums = _op(vecs, blk, None, offset)
        for k in range(len(blk)):
            for q, t in enumerate(_terms(*[v[off[k]:off[k + 1]] for v in vecs], blk[k] < 0)):
                assert abs(sums[k, q] - float(np.sum(t))) <= lens[k] * U * float(np.sum(np.abs(t)))
    lib = cuadmm_amd.load()
    b = np.asarray(blk, np.int32)
    out = np.zeros(6 * b.size)
    short = [v[:-1].copy() for v in vecs]
    assert lib.cuadmm_op_ev_block_stats(short[0].size, *[P(v) for v in short], b.size, P(b), None, 0, P(out)) == -1
    assert "outside the vectors" in lib.cuadmm_last_error().decode()
    bad = b.copy()
    bad[3] = 0
    assert lib.cuadmm_op_ev_block_stats(vecs[0].size, *[P(v.copy()) for v in vecs], b.size, P(bad), None, 0, P(out)) == -1


# ---- the report against the twin ------------------------------------------------------------------------------------------
def tolerances(fx, tw):
    """(tol of out[0:15], tol of per_block) from the twin's numbers: the module docstring"""
    o, pb = tw["out"], tw["per_block"]
    lens = blk_lens(fx.blk)
    tp = np.zeros_like(pb)
    tp[:, 0], tp[:, 2] = 64 * U * pb[:, 0], 64 * U * pb[:, 2]
    tp[:, 1] = 2e-12 * np.sqrt(lens) * pb[:, 0]
    tp[:, 3] = 2e-12 * np.sqrt(lens) * pb[:, 2]
    free = np.asarray(fx.blk) < 0
    tp[free, 1], tp[free, 3] = 0.0, tp[free, 2]
    tp[:, 4] = 64 * U * tw["abs_XS"]
    tp[:, 5] = tw["rd_bound"] + 64 * U * pb[:, 5]
    t = np.zeros(15)
    t[0], t[1] = 64 * U * tw["abs_cx"], 64 * U * tw["abs_by"]
    t[2] = tw["rp_bound"] + 64 * U * o[2]
    t[3] = np.linalg.norm(tw["rd_bound"]) + 64 * U * o[3]
    t[4] = np.linalg.norm(tp[:, 1]) + 64 * U * o[4]
    t[5] = np.linalg.norm(tp[:, 3]) + 64 * U * o[5]
    t[6] = 64 * U * float(np.sum(tw["abs_XS"]))
    t[7], t[8] = 64 * U * o[7], 64 * U * o[8]
    nb, nc, den = 1 + o[7], 1 + o[8], 1 + abs(o[0]) + abs(o[1])
    t[9], t[10], t[11], t[12] = t[2] / nb, t[4] / nb, t[3] / nc, t[5] / nc
    t[13] = 2 * (t[0] + t[1]) / den
    t[14] = (t[6] + t[0] + t[1]) / den
    t[9:15] += 64 * U * np.abs(o[9:15])
    return t, tp


def against_twin(fx, got, X, y, S, what):
    tw = evaluate(fx, X, y, S)
    t, tp = tolerances(fx, tw)
    go = np.array([got[k] for k in KEYS[:15]])
    eo, ep = np.abs(go - tw["out"][:15]), np.abs(got["per_block"] - tw["per_block"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ro, rp = np.where(eo > 0, eo / t, 0.0), np.where(ep > 0, ep / tp, 0.0)
    print("%s: worst error / tolerance: scalars %.3g (%s), per block %s; err1..6 %s; %.3f ms"
          % (what, ro.max(), KEYS[int(np.argmax(ro))], np.array2string(rp.max(axis=0), precision=3), np.array2string(go[9:15], precision=3), got["ms"]))
    assert np.all(ep <= tp), (what, "per_block", np.argwhere(ep > tp), ep[ep > tp], tp[ep > tp])
    assert np.all(eo <= t), (what, [KEYS[i] for i in np.nonzero(eo > t)[0]], eo[eo > t], t[eo > t])
    assert got["ms"] > 0
    return tw, tp


# ---- 2. a known optimum ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_report_at_a_known_optimum(name):
    fx = fixture(name)
    s = solver(fx)
    got = s.evaluate(fx.Xs, fx.ys, fx.Ss)
    tw, tp = against_twin(fx, got, fx.Xs, fx.ys, fx.Ss, name + " optimum")
    assert np.all(np.abs(tw["out"][9:15]) <= 1e-12)
    assert np.all(got["per_block"][:, 1] <= tp[:, 1]) and np.all(got["per_block"][np.asarray(fx.blk) > 0, 3] <= tp[np.asarray(fx.blk) > 0, 3])
    info = s.evaluate_info()
    L = int(blk_lens(fx.blk).sum())
    assert info["calls"] == 1 and 8 * (3 * L + fx.m) <= info["bytes"] and info["aux_bytes"] >= 16 * L
    # vectors: at most 3 L + m doubles (+ m: the column norms, where the y-solve keeps them on the host); the rest: 6 sums per
    # block and per chunk (at most 8 chunks here), three arrays of 256 partials, 8 results, two 8-byte and at most six 4-byte list entries
    # per block, five per chunk
    nb = len(fx.blk)
    assert info["bytes"] <= 8 * (3 * L + 2 * fx.m + 6 * nb + 6 * 8 + 768 + 8 + 2 * nb) + 4 * (6 * nb + 5 * 8)


# ---- 3. known violations --------------------------------------------------------------------------------------------------
def _with_spectrum(n, lam, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    M = (Q * lam) @ Q.T
    return svec((M + M.T) / 2)


def test_report_at_known_violations():
    fx = fixture("A")
    rng = np.random.default_rng(11)
    off = offsets(fx.blk)
    X, y, S = fx.Xs.copy(), fx.ys.copy(), fx.Ss.copy()
    lamX = np.concatenate([[-0.7, -0.2, -0.05], 0.1 + rng.random(67)])           # block 2 (n = 70) of X: three negative eigenvalues
    lamS = np.concatenate([[-1.5, -0.4, -0.01], 0.1 + rng.random(17)])           # block 1 (n = 20) of S
    X[off[2]:off[3]] = _with_spectrum(70, lamX, rng)
    S[off[1]:off[2]] = _with_spectrum(20, lamS, rng)
    S[off[3]:off[4]] = [0.3, -0.4]                                               # the free block: its dual cone is {0}
    y *= 1 + 1e-3 * rng.standard_normal(fx.m)
    s = solver(fx)
    got = s.evaluate(X, y, S)
    tw, tp = against_twin(fx, got, X, y, S, "A violations")
    pb = got["per_block"]
    want_vX, want_vS = np.linalg.norm(lamX[:3]), np.linalg.norm(lamS[:3])
    assert abs(pb[2, 1] - want_vX) <= tp[2, 1] + 1e-13 and abs(pb[1, 3] - want_vS) <= tp[1, 3] + 1e-13      # (1e-13: the hand-made spectrum through QR)
    assert abs(pb[3, 3] - 0.5) <= 64 * U and pb[3, 1] == 0.0
    for k in (0, 1, 3, 4):
        assert pb[k, 1] <= tp[k, 1]                                              # untouched blocks of X
    for k in (0, 2, 4):
        assert pb[k, 3] <= tp[k, 3]
    assert got["err2"] > 0.01 and got["err4"] > 0.01 and got["err3"] > 1e-5 and got["err1"] > 1e-3


# ---- 4. the current iterate -----------------------------------------------------------------------------------------------
def test_report_of_the_current_iterate():
    """100 iterations on B (sGS phase: no best-iterate restore).  evaluate() reads the scaled iterate where it lies; a second, identical
    solver hands out X, y, S (unscaled) and evaluates them as a foreign point (scaled again): every entry moved by at most two roundings,
    so every reported number moves by a few U times the absolute sum it is formed from -- 1e-13 (900 U) relative to that scale: the
    norm itself for norms, ||X_k|| / ||S_k|| for vX_k / vS_k, |C|'|X|, |b|'|y|, |X|'|S| for the inner products, || |A||X| + |b| || and
    || |C| + |A|'|y| + |S| || for the residual norms, 1 for the errors (quotients by 1 + ...).
    errRp of cuadmm_get_state coincides with err1: both are ||normA (b_s - A_s X_s) bscale|| / (1 + ||b||) of the X the solve returns.
    errRd does not coincide with err3: the engine's is formed at the y the last iteration used, while the solve returns the y of one more
    y-solve (the reference's loop solves before it breaks); only its size is comparable."""
    fx = fixture("B")
    a, b = solver(fx), solver(fx)
    for s in (a, b):
        s.solve(100, 1e-12)
    ra = a.evaluate()
    X, y, S = b.X, b.y, b.S
    rb = b.evaluate(X, y, S)
    tw = evaluate(fx, X, y, S)
    off = offsets(fx.blk)
    absA = np.abs(fx.A)
    sc_rp = np.linalg.norm(absA @ np.abs(X) + np.abs(fx.b))
    e_rd = np.abs(fx.C) + absA.T @ np.abs(y) + np.abs(S)
    sc_rd = np.array([np.linalg.norm(e_rd[off[k]:off[k + 1]]) for k in range(len(fx.blk))])
    pa, pbk = ra["per_block"], rb["per_block"]
    scale_pb = np.stack([pbk[:, 0], pbk[:, 0], pbk[:, 2], pbk[:, 2], tw["abs_XS"], sc_rd], axis=1)
    assert np.all(np.abs(pa - pbk) <= 1e-13 * scale_pb), np.abs(pa - pbk) / scale_pb
    scale = {"pobj": tw["abs_cx"], "dobj": tw["abs_by"], "norm_Rp": sc_rp, "norm_Rd": np.linalg.norm(sc_rd), "vX": rb["per_block"][:, 0].max() * np.sqrt(len(fx.blk)),
             "vS": rb["per_block"][:, 2].max() * np.sqrt(len(fx.blk)), "XS": float(np.sum(tw["abs_XS"])), "norm_b": rb["norm_b"], "norm_C": rb["norm_C"]}
    for k in KEYS[:15]:
        sc = scale.get(k, 1.0)
        print("%-8s %.17g | %.17g  difference / scale %.3g" % (k, ra[k], rb[k], abs(ra[k] - rb[k]) / sc))
        assert abs(ra[k] - rb[k]) <= 1e-13 * sc, k
    against_twin(fx, rb, X, y, S, "B after 100 iterations")
    st = a.state()
    print("errRp %.17g, err1 %.17g; errRd %.3e, err3 %.3e" % (st["errRp"], ra["err1"], st["errRd"], ra["err3"]))
    assert abs(ra["err1"] - st["errRp"]) <= 1e-10 * st["errRp"]
    assert abs(ra["norm_b"] + 1 - st["norm_borg"]) <= 4 * U * st["norm_borg"] and abs(ra["norm_C"] + 1 - st["norm_Corg"]) <= 4 * U * st["norm_Corg"]


# ---- 5. no side effects ---------------------------------------------------------------------------------------------------
def _traj(s):
    return [s.info_arr(k).copy() for k in INFO] + [s.X, s.y, s.S]


@pytest.mark.parametrize("mode", ["sgs", "admm", "accel"])
def test_the_call_leaves_the_iteration_alone(mode):
    fx = fixture("A")
    rng = np.random.default_rng(2)
    foreign = (rng.standard_normal(fx.L), rng.standard_normal(fx.m), rng.standard_normal(fx.L))
    sw = 0 if mode == "admm" else int(1.1e4)
    runs = []
    for call in (True, False):
        s = solver(fx, {"accel": 5} if mode == "accel" else None)
        s.solve(60, 0.0, switch_admm=sw)
        if call:
            r = s.evaluate()
            assert np.isfinite([r[k] for k in KEYS]).all()
            s.evaluate(*foreign)
        s.solve(60, 0.0, switch_admm=sw, if_first=False)
        runs.append(_traj(s))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---- 6. the engine's other plans ------------------------------------------------------------------------------------------
def _psd_ish_point(fx, seed):
    """X, S: G G' / n minus a shift that leaves a few negative eigenvalues; the free blocks and y random"""
    rng = np.random.default_rng(seed)
    off = offsets(fx.blk)
    X, S = np.zeros(fx.L), np.zeros(fx.L)
    for k, n in enumerate(fx.blk):
        for v in (X, S):
            if n < 0:
                v[off[k]:off[k + 1]] = rng.standard_normal(-n)
            else:
                G = rng.standard_normal((n, n))
                v[off[k]:off[k + 1]] = svec(G @ G.T / n - 0.05 * np.eye(n))
    return X, rng.standard_normal(fx.m), S


def _dense_fixture(p):
    A = np.zeros((p.con_num, p.vec_len))
    for j in range(p.con_num):
        sl = slice(p.At_col_ptrs[j], p.At_col_ptrs[j + 1])
        A[j, p.At_row_ids[sl]] = p.At_vals[sl]
    b, Cv = np.zeros(p.con_num), np.zeros(p.vec_len)
    b[p.b_idx], Cv[p.C_idx] = p.b_vals, p.C_vals
    return Fixture(p.blk, A, b, Cv)


def test_report_on_closed_blocks():
    """256 blocks of 8 with 2 local constraints each, the smallest the closed path accepts: it needs the device-side forest solve, which
    starts at 256 trees of the elimination forest (engine.hip: init_solve_plan, init_closed), one tree per block here.  Every block is
    closed (the blocks solve for their own multipliers, the iteration keeps no stand-alone A X product); the report forms A X from the
    engine's whole A, before a solve and on the iterate behind one"""
    p = synthetic.make_synthetic([8] * 256, cons_per_block=2, seed=5)
    fx = _dense_fixture(p)
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(cuadmm_amd.Problem(p.vec_len, p.con_num, p.blk, p.At_col_ptrs, p.At_row_ids, p.At_vals, p.b_idx, p.b_vals, p.C_idx, p.C_vals))
    assert s.counters()["closed_blocks"] == 1
    X, y, S = _psd_ish_point(fx, 3)
    against_twin(fx, s.evaluate(X, y, S), X, y, S, "closed blocks, before a solve")
    s.solve(40, 0.0, switch_admm=10)
    r = s.evaluate()
    Xi, yi, Si = s.X, s.y, s.S
    tw = evaluate(fx, Xi, yi, Si)
    assert abs(r["norm_Rp"] - tw["norm_Rp"]) <= tw["rp_bound"] + 1e-13 * np.linalg.norm(np.abs(fx.A) @ np.abs(Xi) + np.abs(fx.b))
    against_twin(fx, s.evaluate(X, y, S), X, y, S, "closed blocks, behind a solve")


def test_report_after_updates_and_with_gap_check():
    fx = fixture("A")
    rng = np.random.default_rng(9)
    X, y, S = _psd_ish_point(fx, 4)
    s = solver(fx)
    s.solve(20, 0.0)
    fb = Fixture(fx.blk, fx.A, fx.b * (1 + 0.3 * rng.standard_normal(fx.m)), fx.C + 0.2 * rng.standard_normal(fx.L))
    bi, ci = np.nonzero(fb.b)[0], np.nonzero(fb.C)[0]
    s.update_bC(bi, fb.b[bi], ci, fb.C[ci])
    against_twin(fb, s.evaluate(X, y, S), X, y, S, "A after update_bC")
    fa = Fixture(fx.blk, fx.A * (1 + 0.2 * rng.standard_normal(fx.A.shape)), fb.b, fb.C)
    s.update_A(amd(fa).At_csc_vals)
    against_twin(fa, s.evaluate(X, y, S), X, y, S, "A after update_A")
    Xi, yi, Si = s.X, s.y, s.S                                     # the warm start the update left, in the caller's units
    against_twin(fa, s.evaluate(), Xi, yi, Si, "A after update_A, the resident point")
    g = cuadmm_amd.SDPSolver(verbose=False, options={"gap_check": 10})
    g.set_trace_bounds(fx.R)
    g.init_problem(amd(fx))
    g.solve(30, 0.0)
    against_twin(fx, g.evaluate(X, y, S), X, y, S, "A with gap_check = 10")
    assert g.gap_info()["checks"] == 3


def test_the_report_and_the_bound_share_one_task_list():
    """Fixture B (odd offsets, a free block, a wavefront-owned block) at one random point, set with set_XyS: a handle that runs lower_bound()
    and then evaluate(), one that runs them the other way round, and two fresh handles with one call each.  The per-block task lists
    on the device are built once per handle by whichever call comes first (csrc/report_plans.h: BlockTasksDev): every number but ms is the
    same to the bit in all three, and each call reports the bytes it would report alone, the lists' included.  The bound's figure
    contains the auxiliary projector's, whose plan is sized from the device's free memory around its build and is no function of the
    handle alone: it is compared without them (evaluate_info's aux_bytes; the lone bound's handle evaluates afterwards to learn them)."""
    fx = fixture("B")
    rng = np.random.default_rng(23)
    X, y, S = rng.standard_normal(fx.L), rng.standard_normal(fx.m), rng.standard_normal(fx.L)

    def handle():
        s = solver(fx)
        s.set_trace_bounds(fx.R)
        s.set_XyS(X, y, S)
        return s

    def own_bytes(s, lb):
        return lb["bytes"] - s.evaluate_info()["aux_bytes"]

    s1, s2, s3b, s3e = handle(), handle(), handle(), handle()
    lb1 = s1.lower_bound(per_block=True)
    ev1 = s1.evaluate()
    ev2 = s2.evaluate()
    lb2 = s2.lower_bound(per_block=True)
    lb3 = s3b.lower_bound(per_block=True)
    ev3 = s3e.evaluate()
    evb = [s.evaluate_info()["bytes"] for s in (s1, s2, s3e)]
    s3b.evaluate()
    lbb = [own_bytes(s, lb) for s, lb in ((s1, lb1), (s2, lb2), (s3b, lb3))]
    print("bytes: evaluate %s, lower_bound without the projector %s (with it %s)" % (evb, lbb, [lb["bytes"] for lb in (lb1, lb2, lb3)]))
    for lb in (lb2, lb3):
        for k in lb1:
            if k not in ("ms", "bytes"):
                assert np.array_equal(lb1[k], lb[k]), k
    for ev in (ev2, ev3):
        for k in ev1:
            if k != "ms":
                assert np.array_equal(ev1[k], ev[k]), k
    assert np.isfinite(lb1["lower_bound"]) and np.isfinite([ev1[k] for k in KEYS]).all()
    assert evb[0] == evb[1] == evb[2] and lbb[0] == lbb[1] == lbb[2] and min(evb + lbb) > 0
    assert s3b.evaluate_info()["bytes"] == evb[0] and s3e.gap_info()["bytes"] == 0.0


def _one_y(fx, a, b, what):
    """a reports on its resident point without handing it out; b, in the same state, hands it out and numpy forms the numbers (the
    inner product and C - A'y in longdouble, so that the bounds below are spent on the engine alone)"""
    lb, ev, lm = a.lower_bound(per_block=True), a.evaluate(), a.lambda_min("dual")
    X, y, S = b.X, b.y, b.S
    off = offsets(fx.blk)
    by = float(np.sum(fx.b.astype(LD) * y.astype(LD)))
    sc_by = float(np.abs(fx.b) @ np.abs(y))
    Sh = np.asarray(fx.C.astype(LD) - fx.A.T.astype(LD) @ y.astype(LD), np.float64)
    e = np.abs(fx.C) + np.abs(fx.A).T @ np.abs(y)
    sc = np.array([np.linalg.norm(e[off[k]:off[k + 1]]) for k in range(len(fx.blk))])
    for name, got in (("evaluate dobj", ev["dobj"]), ("lower_bound bty", lb["bty"]), ("lower_bound", lb["lower_bound"]), ("lambda_min lower_bound", lm["lower_bound"])):
        print("%s, %-22s %.17g | numpy %.17g  difference / |b|'|y| %.3g" % (what, name, got, by, abs(got - by) / sc_by))
        assert abs(got - by) <= 1e-13 * sc_by, (what, name)
    nS = np.array([np.linalg.norm(Sh[off[k]:off[k + 1]]) for k in range(len(fx.blk))])
    lam = np.array([np.linalg.eigvalsh(smat(Sh[off[k]:off[k + 1]], int(n)))[0] if n > 0 else np.inf for k, n in enumerate(fx.blk)])
    psd = np.asarray(fx.blk) > 0
    print("%s: worst | ||S^_k|| - numpy | / scale %.3g, worst (lo_k - lambda_min_k) / scale %.3g"
          % (what, float(np.max(np.abs(lb["norm_S"] - nS) / sc)), float(np.max((lm["lo"][psd] - lam[psd]) / sc[psd]))))
    assert np.all(np.abs(lb["norm_S"] - nS) <= 1e-13 * sc), what
    assert np.all(lm["lo"][psd] <= lam[psd] + 1e-13 * sc[psd]), what
    against_twin(fx, ev, X, y, S, what)


@pytest.mark.parametrize("name", ["A", "closed"])
def test_the_three_reports_read_one_y_in_every_resident_state(name):
    """lower_bound(), evaluate() and lambda_min("dual") stage the resident y through one routine (csrc/engine_reports.hip: stage_scaled_y), whose
    branches are the states y can be in: in the caller's units on the host (1: behind set_XyS), scaled behind a solve (2; on the host
    with the y-solve there: fixture A, on the device with it there: 256 blocks of 8, test_report_on_closed_blocks), in the caller's
    units on the device only (3: behind update_bC(keep_iterate) on the device y-solve, before any getter) and on the host again (4: a
    getter has run).  Trace bounds of zero: the penalty vanishes and all three expose b'y.  Bounds: the rule of
    test_report_of_the_current_iterate -- every entry of y moved by at most two roundings, so a number moves by a few U times the
    absolute sum it is formed from, 1e-13 (900 U) relative to |b|'|y| for b'y and to ||(|C| + |A|'|y|)_k|| for block k of C - A'y, its
    norm and (Weyl) its smallest eigenvalue."""
    if name == "A":
        fx = fixture("A")
        prob, where = amd(fx), (0, 2)                              # cuadmm_get_counters: the y-solve on the host (2: hybrid)
    else:
        p = synthetic.make_synthetic([8] * 256, cons_per_block=2, seed=5)
        fx = _dense_fixture(p)
        prob, where = cuadmm_amd.Problem(p.vec_len, p.con_num, p.blk, p.At_col_ptrs, p.At_row_ids, p.At_vals, p.b_idx, p.b_vals, p.C_idx, p.C_vals), (1, 3)
    rng = np.random.default_rng(31)
    X0, y0, S0 = rng.standard_normal(fx.L), rng.standard_normal(fx.m), rng.standard_normal(fx.L)
    fb = Fixture(fx.blk, fx.A, fx.b * (1 + 0.3 * rng.standard_normal(fx.m)), fx.C + 0.2 * rng.standard_normal(fx.L))
    bi, ci = np.nonzero(fb.b)[0], np.nonzero(fb.C)[0]

    def pair():
        hs = []
        for _ in range(2):
            s = cuadmm_amd.SDPSolver(verbose=False)
            s.set_trace_bounds(np.zeros(len(fx.blk)))
            s.init_problem(prob)
            assert int(s.counters()["dev_solve"]) in where
            hs.append(s)
        return hs

    a, b = pair()
    for s in (a, b):
        s.set_XyS(X0, y0, S0)
    _one_y(fx, a, b, name + " state 1 (set_XyS)")
    for s in (a, b):
        s.solve(30, 0.0)
    _one_y(fx, a, b, name + " state 2 (behind a solve)")
    a, b = pair()
    for s in (a, b):
        s.solve(30, 0.0)
        s.update_bC(bi, fb.b[bi], ci, fb.C[ci], keep_iterate=True)
    _one_y(fb, a, b, name + " state 3 (behind update_bC, no getter)")
    assert a.y.size == fx.m                                        # one getter: y is on the host again
    _one_y(fb, a, b, name + " state 4 (behind update_bC and a getter)")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_solver_as_it_was():
    fx = fixture("B")
    bad_X, bad_y = fx.Xs.copy(), fx.ys.copy()
    bad_X[17], bad_y[3] = np.nan, np.inf
    runs = []
    for call in (True, False):
        s = solver(fx)
        s.solve(40, 0.0)
        if call:
            for kw, why in (({"X": bad_X}, r"X\[17\] is not finite"), ({"y": bad_y}, r"y\[3\] is not finite")):
                with pytest.raises(cuadmm_amd.CuadmmError, match=why) as e:
                    s.evaluate(**kw)
                assert e.value.code == -1
            assert s.evaluate_info()["calls"] == 0
        s.solve(40, 0.0, if_first=False)
        runs.append(_traj(s))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    # world = 2 (rank 0 of two, the hook left empty: the run is not a solve of the problem, only a state to continue from)
    runs = []
    for call in (True, False):
        s = cuadmm_amd.SDPSolver(verbose=False, rank=0, world=2)
        s.set_allreduce(lambda ptr, count, stream: None)
        s.init_problem(amd(fx))
        s.solve(20, 0.0)
        if call:
            with pytest.raises(cuadmm_amd.CuadmmError, match="works on one rank.*not all-reduced") as e:
                s.evaluate()
            assert e.value.code == -1
        s.solve(20, 0.0, if_first=False)
        runs.append(_traj(s))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---- 8. command line ------------------------------------------------------------------------------------------------------
def _write_txt(d, fx):
    os.makedirs(d)
    with open(d + "blk.txt", "w") as f:
        for n in fx.blk:
            f.write("%s %d\n" % ("s" if n > 0 else "u", abs(int(n))))
    with open(d + "con_num.txt", "w") as f:
        f.write("%d\n" % fx.m)
    r, c, v = fx.coo()
    with open(d + "At.txt", "w") as f:
        for i, j, x in zip(r, c, v):
            f.write("%d %d %.17g\n" % (i, j, x))
    for nm, vec in (("b", fx.b), ("C", fx.C)):
        with open(d + nm + ".txt", "w") as f:
            for i in np.nonzero(vec)[0]:
                f.write("%d 0 %.17g\n" % (i, vec[i]))


def _same_report(side, r):
    for k in KEYS[:15]:
        assert side[k] == r[k], (k, side[k], r[k])
    assert np.array_equal(np.array(side["per_block"]), r["per_block"]) and side["ms"] > 0


def test_cli_kkt(tmp_path):
    fx = fixture("B")
    d, d2 = str(tmp_path / "prob") + "/", str(tmp_path / "point") + "/"
    _write_txt(d, fx)
    exe = os.path.join(ROOT, "cuadmm_amd", "lib", "cuadmm_exe")
    lib = cuadmm_amd.load()
    prob = cuadmm_amd.Problem.from_txt(d)
    assert np.array_equal(prob.blk_vals, np.asarray(fx.blk, np.int32))
    # --kkt behind a solve with the command line's parameters
    js = str(tmp_path / "kkt.json")
    r = subprocess.run([exe, d, "--kkt", "--max_iter=150", "--stop_tol=1e-12", "--quiet", "--json=" + js], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "KKT report" in r.stdout and "DIMACS: err1" in r.stdout
    with open(js) as f:
        side = json.load(f)
    s = cuadmm_amd.SDPSolver(verbose=False, profile=True)
    s.init_problem(prob)
    s.solve(150, 1e-12, 0, 50, 100, 5000, 1.05)
    _same_report(side["kkt"], s.evaluate())
    assert side["iterations"] == 150
    r = subprocess.run([exe, d, "--max_iter=20", "--quiet", "--json=" + js], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "KKT report" not in r.stdout
    with open(js) as f:
        assert "kkt" not in json.load(f)
    # --kkt-point: X.txt and y.txt as cuadmm_write_dense_txt writes them, S.txt missing (zero)
    os.makedirs(d2)
    rng = np.random.default_rng(1)
    X, y = fx.Xs + 0.01 * rng.standard_normal(fx.L), fx.ys.copy()
    for nm, vec in (("X", X), ("y", y)):
        assert lib.cuadmm_write_dense_txt((d2 + nm + ".txt").encode(), P(vec), vec.size) == 0
    Xr, yr = np.loadtxt(d2 + "X.txt"), np.loadtxt(d2 + "y.txt")          # what the file holds (32 decimals)
    r = subprocess.run([exe, d, "--kkt-point=" + d2, "--quiet", "--json=" + js], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "KKT report" in r.stdout
    with open(js) as f:
        side = json.load(f)
    q = cuadmm_amd.SDPSolver(verbose=False)
    q.init_problem(prob)
    _same_report(side["kkt"], q.evaluate(Xr, yr, np.zeros(fx.L)))
    assert "iterations" not in side                                       # the point run solves nothing
