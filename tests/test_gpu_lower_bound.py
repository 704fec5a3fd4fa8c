"""The certified lower bound from trace bounds on the GPU ("Certified lower bound"; csrc/lower_bound.hip;
csrc/engine_reports.hip: lb_eval, lb_step): the per-block norm kernels against numpy, cuadmm_lower_bound against the numpy twin
(tests/_lower_bound_twin.py) on problems with a known optimum p*, its absence of side effects, option "gap_check" against the twin's
rule, the refusals and the command line.

Tolerances.  A per-block sum of squares: len_k 2^-53 sum |terms|, which holds for every summation order.  nu_k against the twin:
2e-12 sqrt(len_k) ||S^_k||_F, twice the projection kernels' contract.  LB against the twin: the sum of those times R_k plus
64 2^-53 (|b'y| + sum R_k ||S^_k||) (lb_tolerance).  At y*, p* - LB(y*) = sum R_k nubar_k is the bound's own rounding term
sum R_k kLbProjErr sqrt(len_k) ||S*_k||_F (nu_k = 0 there in exact arithmetic) plus those tolerances.
"""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from tests._lower_bound_twin import (PROJ_ERR, blk_lens, form_error, gap, lb_sensitivity, lb_tolerance, lower_bound, make_opt_fixture,
                                     nu_tolerance, twin_solve)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
U = 2.0 ** -53
INFO = ("pobj", "dobj", "errRp", "errRd", "relgap", "sig")
BLK_A, M_A = [3, 20, 70, -2, 130], 40                     # register, one-wavefront, LDS and cluster classes, a free block
BLK_B, M_B = [1] * 40 + [2, 5, 8, -3, 33], 30             # odd offsets
_fx, _solved = {}, {}


def fixture(name):
    if name not in _fx:
        _fx[name] = make_opt_fixture(BLK_A, M_A, 1) if name == "A" else make_opt_fixture(BLK_B, M_B, 1)
    return _fx[name]


def amd(fx):
    r, c, v = fx.coo()
    bi, ci = np.nonzero(fx.b)[0], np.nonzero(fx.C)[0]
    return cuadmm_amd.Problem.from_coo(fx.blk, fx.m, r, c, v, bi, fx.b[bi], ci, fx.C[ci])


def solver(fx, options=None, bounds=True, **kw):
    s = cuadmm_amd.SDPSolver(verbose=False, options=options, **kw)
    if bounds:
        s.set_trace_bounds(fx.R)
    s.init_problem(amd(fx))
    return s


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------
OP_LISTS = {
    "mixed": [1] * 37 + [2, 3, 5, 8] + [-1, -7] + [9, 31, 64, 65] + [-130] + [200],        # 200: 20 100 slots, three chunks
    "n600": [600],                                                                          # 180 300 slots: 23 chunks
    "many3": [3] * 20000,
}


def _op(M, Pv, blk, offs, R, offset):
    lib = cuadmm_amd.load()
    blk = np.asarray(blk, np.int32)
    M, Pv = M.copy(), Pv.copy()
    pairs, comb = np.zeros(2 * blk.size), np.zeros(3)
    rc = lib.cuadmm_op_lb_block_norms(M.size, P(M), P(Pv), blk.size, P(blk), P(offs), P(R), offset, P(pairs), P(comb))
    assert rc == 0, lib.cuadmm_last_error()
    return M, Pv, pairs.reshape(-1, 2), comb


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", list(OP_LISTS))
def test_block_norms_kernel(name, offset):
    blk = OP_LISTS[name]
    rng = np.random.default_rng(len(blk) + offset)
    lens = blk_lens(blk)
    gaps = rng.integers(0, 4, size=len(blk))                     # arbitrary offsets: up to three slots between two blocks, NaN in them
    offs = (np.concatenate([[0], np.cumsum(lens + gaps)[:-1]]) + 1).astype(np.int64)
    n = int(offs[-1] + lens[-1] + 2)
    M, Pv = np.full(n, np.nan), np.full(n, np.nan)
    for o, ln in zip(offs, lens):
        M[o:o + ln] = rng.standard_normal(ln) * 10.0 ** rng.integers(-3, 4)
        Pv[o:o + ln] = rng.standard_normal(ln)
    R = rng.random(len(blk)) + 0.1
    M1, P1, pairs, comb = _op(M, Pv, blk, offs, R, offset)
    assert np.array_equal(M1, M, equal_nan=True) and np.array_equal(P1, Pv, equal_nan=True)      # nothing is written to the vectors
    worst = 0.0
    for k, (o, ln) in enumerate(zip(offs, lens)):
        for q, v in enumerate((M, Pv)):
            t = v[o:o + ln] * v[o:o + ln]
            want, bound = math.fsum(t), ln * U * math.fsum(t)
            worst = max(worst, abs(pairs[k, q] - want) / bound)
            assert abs(pairs[k, q] - want) <= bound, (k, blk[k], q, pairs[k, q], want)
    # the combine kernel on the device's pairs: nblk terms added in a fixed order, two square roots and three products per term
    nubar = np.sqrt(pairs[:, 1]) + np.where(np.array(blk) >= 0, PROJ_ERR * np.sqrt(lens) * np.sqrt(pairs[:, 0]), 0.0)
    terms = R * nubar
    print("%s offset %d: worst sum error / bound %.3f; combined %.17g, numpy %.17g" % (name, offset, worst, comb[0], math.fsum(terms)))
    assert abs(comb[0] - math.fsum(terms)) <= (len(blk) + 8) * U * math.fsum(terms)
    assert int(comb[1]) == int(np.argmax(terms)) and abs(comb[2] - terms.max()) <= 8 * U * terms.max()
    _, _, pairs2, comb2 = _op(M, Pv, blk, offs, R, offset)
    assert np.array_equal(pairs, pairs2) and np.array_equal(comb, comb2)                          # bit-identical from run to run


def test_block_norms_kernel_consecutive_blocks():
    """offs = NULL: one block behind the other, as the engine lays them out"""
    blk = OP_LISTS["mixed"]
    lens = blk_lens(blk)
    rng = np.random.default_rng(7)
    M, Pv, R = rng.standard_normal(int(lens.sum())), rng.standard_normal(int(lens.sum())), np.ones(len(blk))
    off = np.concatenate([[0], np.cumsum(lens)])
    for offset in (0, 1):
        _, _, pairs, _ = _op(M, Pv, blk, None, R, offset)
        for k in range(len(blk)):
            for q, v in enumerate((M, Pv)):
                t = v[off[k]:off[k + 1]] ** 2
                assert abs(pairs[k, q] - math.fsum(t)) <= lens[k] * U * math.fsum(t)


# ---- 2., 3. the bound at an arbitrary y and at y* -------------------------------------------------------------------------
def _against_twin(fx, got, tw, R, what, extra=None):
    tol_nu = nu_tolerance(fx, tw["norm_S"]) + (0.0 if extra is None else extra)
    err = np.abs(got["nu"] - tw["nu"])
    print("%s: LB %.15g (twin %.15g, tolerance %.3g), worst nu error / tolerance %.3g, %.3f ms, %.0f bytes"
          % (what, got["lower_bound"], tw["lb"], lb_tolerance(fx, tw, R), float(np.max(err / np.maximum(tol_nu, 1e-300))), got["ms"], got["bytes"]))
    assert np.all(err <= tol_nu), (what, err, tol_nu)
    assert np.all(np.abs(got["norm_S"] - tw["norm_S"]) <= 64 * U * tw["norm_S"] + form_error(fx, tw["y"]))     # (the issue of forming S^ itself)
    tol = lb_tolerance(fx, tw, R) + (0.0 if extra is None else float(np.sum(R * extra)))
    assert abs(got["lower_bound"] - tw["lb"]) <= tol
    assert abs(got["bty"] - tw["bty"]) <= 64 * U * abs(tw["bty"]) + 64 * U * float(np.abs(fx.b) @ np.abs(tw["y"]))
    assert got["worst_block"] == tw["worst"] and got["bytes"] > 0


@pytest.mark.parametrize("name", ["A", "B"])
def test_bound_at_an_arbitrary_y(name):
    fx = fixture(name)
    s = solver(fx)
    y = np.random.default_rng(5).standard_normal(fx.m)            # far from y*
    s.set_XyS(y=y)
    got = s.lower_bound(per_block=True)
    tw = dict(lower_bound(fx, y, fx.R), y=y)
    _against_twin(fx, got, tw, fx.R, name + " random y")
    assert got["lower_bound"] <= fx.pstar
    assert got["gap"] == gap(s.state()["pobj"], got["lower_bound"])


@pytest.mark.parametrize("name", ["A", "B"])
def test_bound_is_tight_at_the_optimal_y(name):
    fx = fixture(name)
    s = solver(fx)
    s.set_XyS(y=fx.ys)
    got = s.lower_bound()
    tw = lower_bound(fx, fx.ys, fx.R)
    own = float(np.sum(fx.R * (tw["nubar"] - tw["nu"])))           # the bound's rounding term: sum R_k kLbProjErr sqrt(len_k) ||S*_k||_F
    print("%s: p* - LB(y*) = %.3e, the bound's rounding term %.3e, tolerances %.3e" % (name, fx.pstar - got["lower_bound"], own, lb_tolerance(fx, tw, fx.R)))
    assert got["lower_bound"] <= fx.pstar
    assert fx.pstar - got["lower_bound"] <= own + lb_tolerance(fx, tw, fx.R)


# ---- 4. after a solve -----------------------------------------------------------------------------------------------------
def solved(name):
    if name not in _solved:
        s = solver(fixture(name))
        s.solve(3000, 1e-6)
        _solved[name] = s
    return _solved[name]


@pytest.mark.parametrize("name", ["A", "B"])
def test_bound_after_a_solve(name):
    fx, s = fixture(name), solved(name)
    first = s.lower_bound(per_block=True)                          # on the scaled iterate the solve left
    y = s.y                                                        # (brings the iterate to the caller's units)
    again = s.lower_bound(per_block=True)
    tw = dict(lower_bound(fx, y, fx.R), y=y)
    extra = form_error(fx, y)
    for what, got in (("scaled state", first), ("caller's units", again)):
        _against_twin(fx, got, tw, fx.R, "%s after %d iterations, %s" % (name, s.info_iter_num, what), extra)
        assert got["lower_bound"] <= fx.pstar
    print("%s: p* %.12g, LB %.12g, pobj %.12g, certified gap %.3e" % (name, fx.pstar, first["lower_bound"], s.state()["pobj"], first["gap"]))
    # a smaller feasible set: the bound holds for it (X* is no longer inside, so it may exceed p*)
    k = int(np.argmax(np.array(fx.blk)))
    R2 = fx.R.copy()
    R2[k] = 0.4 * fx.R[k] / 1.5
    s.set_trace_bounds(R2)
    small = s.lower_bound()
    tw2 = lower_bound(fx, y, R2)
    assert np.isfinite(small["lower_bound"]) and small["lower_bound"] <= tw2["lb"] + lb_tolerance(fx, tw2, R2) + float(np.sum(R2 * extra))
    assert small["lower_bound"] >= first["lower_bound"]
    with pytest.raises(RuntimeError, match="finite and not negative"):
        s.set_trace_bounds(-R2)
    assert s.lower_bound()["lower_bound"] == small["lower_bound"]  # a refusal leaves the bounds as they were
    s.set_trace_bounds(fx.R)


# ---- 5. no side effects ---------------------------------------------------------------------------------------------------
def _traj(s):
    return [s.info_arr(k).copy() for k in INFO] + [s.X, s.y, s.S]


@pytest.mark.parametrize("name", ["A", "B"])
def test_the_call_leaves_the_iteration_alone(name):
    fx = fixture(name)
    runs = []
    for call in (False, True):
        s = solver(fx)
        if call:
            s.lower_bound()                                        # before the first solve
        s.solve(100, 1e-6)
        if call:
            s.lower_bound(per_block=True)
        s.solve(100, 1e-6, if_first=False)
        runs.append(_traj(s))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["A", "B"])
def test_gap_check_without_a_verdict_is_the_run_with_the_option_off(name):
    fx = fixture(name)
    off = solver(fx)
    on = solver(fx, {"gap_check": 10, "gap_tol": 1e-30})
    for s in (off, on):
        s.solve(200, 1e-6)
    for a, b in zip(_traj(off), _traj(on)):
        assert np.array_equal(a, b)
    gi, st = on.gap_info(), on.status()
    print(name, gi, st)
    assert st["status"] == off.status()["status"] and st["status"] in (1, 2) and off.gap_info()["checks"] == 0
    assert gi["checks"] == on.info_iter_num // 10 and gi["verdict_iteration"] == 0 and gi["ms"] > 0 and gi["bytes"] > 0
    assert gi["best_lower_bound"] >= gi["last_lower_bound"] and gi["best_iteration"] % 10 == 0 and 10 <= gi["best_iteration"] <= on.info_iter_num
    assert gi["best_lower_bound"] <= fx.pstar
    # the recorded bounds are the twin's: the engine follows the oracle's iteration to 1e-9 relative (the parity bound of
    # tests/test_gpu_solver.py), and lb_sensitivity bounds what a relative change of y does to LB
    t = twin_solve(fx, fx.R, 10, 1e-30, 200, 1e-6)
    assert len(t.checks) == gi["checks"] and t.best[1] == gi["best_iteration"]
    ib = [c[0] for c in t.checks].index(t.best[1])
    for what, got, want, y in (("best", gi["best_lower_bound"], t.best[0], t.ys[ib]), ("last", gi["last_lower_bound"], t.checks[-1][1], t.ys[-1])):
        tol = 1e-9 * lb_sensitivity(fx, y, fx.R)
        print("%s LB %.15g, twin %.15g, difference %.3e, tolerance %.3e" % (what, got, want, abs(got - want), tol))
        assert abs(got - want) <= tol


def test_the_bound_and_the_infeasibility_check_share_one_projector():
    """Fixture A (a free block, PSD blocks of the register, one-wavefront, LDS and cluster classes) with trace bounds and infeas_check = 10:
    the check and cuadmm_lower_bound project through the same auxiliary plan and work vectors (csrc/report_plans.h: AuxProj).  Neither
    sees the other: the trajectory is that of a handle with neither feature, both bounds are those of a handle without the check.
    stop_tol = 0: in each solve every multiple of the period behind the first (the snapshot) is a check, 5 of them.  That one of the
    first five passed a sign test and projected shows in the bytes: the plan is built at the first projection, and without it the check holds
    3 L + 4 m doubles of vectors (its own two snapshots, dy, A dX; the projector's two work vectors and, at most, its copy of b), the
    2 048 + 8 doubles of its reduction and nothing else."""
    fx = fixture("A")
    L, m = int(blk_lens(fx.blk).sum()), fx.m
    plain, bound, both = solver(fx, bounds=False), solver(fx), solver(fx, {"infeas_check": 10})
    lbs = {}
    for s in (plain, bound, both):
        s.solve(60, 0.0)
        if s is both:
            st = s.status()
            print("after the first solve:", st, "vectors alone %d bytes" % (8 * (3 * L + 4 * m + 2056)))
            assert st["status"] == 2 and st["checks"] == 5 and st["ms"] > 0
            assert st["bytes"] > 8 * (3 * L + 4 * m + 2056)
        if s is not plain:
            lbs[s] = [s.lower_bound(per_block=True)]
        s.solve(60, 0.0, if_first=False)
        if s is not plain:
            lbs[s].append(s.lower_bound(per_block=True))
    for a, b in zip(_traj(plain), _traj(both)):
        assert np.array_equal(a, b)
    for want, got in zip(lbs[bound], lbs[both]):
        print("LB %.15g | %.15g" % (want["lower_bound"], got["lower_bound"]))
        for k in want:
            if k not in ("ms", "bytes"):
                assert np.array_equal(want[k], got[k]), k
        assert got["bytes"] > 0 and got["ms"] > 0
    assert both.status()["checks"] == 5 and both.status()["status"] == 2
    for s in (plain, bound, both):                                 # no projection of either plan hit the QL sweep cap (a call would have failed)
        assert s.state()["eig_not_converged"] == 0


# ---- 6. the verdict -------------------------------------------------------------------------------------------------------
GAP_TOL = 1e-3


def test_gap_verdict_ends_the_solve():
    """Fixture A, seed 1, gap_check = 50, gap_tol = 1e-3, stop_tol = 1e-6.  In the twin (CPU): g = 3.358e-3 at iteration 200 (>= 1.25 tol)
    and g = 2.707e-4 at iteration 250 (<= 0.8 tol), errRp = 1.2e-6 there: the verdict falls at iteration 250 with margin on both sides."""
    fx = fixture("A")
    t = twin_solve(fx, fx.R, 50, GAP_TOL, 3000, 1e-6)
    print("twin:", t.status, t.iteration, ["%d: g %.4e" % (c[0], c[2]) for c in t.checks])
    assert t.status == 5 and t.checks[-1][2] <= 0.8 * GAP_TOL and t.checks[-2][2] >= 1.25 * GAP_TOL and t.checks[-1][3] <= 0.8 * GAP_TOL
    s = solver(fx, {"gap_check": 50, "gap_tol": GAP_TOL})
    s.solve(3000, 1e-6)
    st, gi = s.status(), s.gap_info()
    print("engine:", st, gi)
    assert st["status"] == 5 and st["name"] == "certified_gap" and st["iteration"] == t.iteration == s.info_iter_num
    assert gi["verdict_iteration"] == t.iteration and gi["checks"] == t.iteration // 50 and gi["last_gap"] <= GAP_TOL
    assert gi["best_lower_bound"] >= gi["last_lower_bound"] and gi["last_lower_bound"] <= fx.pstar
    after = s.lower_bound()                                        # X, y, S are the verdict's iterate
    assert abs(after["lower_bound"] - gi["last_lower_bound"]) <= 1e-12 * (abs(after["bty"]) + after["penalty"])
    assert abs(after["gap"] - gi["last_gap"]) <= 1e-12
    # bounds set, option off: the solve ends as it did before
    q = solver(fx)
    q.solve(3000, 1e-6)
    assert q.status()["status"] in (1, 2) and q.info_iter_num > t.iteration and q.gap_info()["checks"] == 0


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    fx = fixture("B")
    p = amd(fx)
    for opts, kw, why in (({"gap_check": 50, "accel": 4}, {}, "accel = 4"), ({"gap_check": 50, "infeas_check": 50}, {}, "infeas_check = 50"),
                          ({"gap_check": 50}, {"eig_rank": 2}, "eig_rank = 2"), ({"gap_check": 50}, {"world": 2}, "world = 2")):
        s = cuadmm_amd.SDPSolver(verbose=False, options=opts, **kw)
        s.set_trace_bounds(fx.R)
        with pytest.raises(RuntimeError, match="gap_check.*" + why):
            s.init_problem(p)
    s = cuadmm_amd.SDPSolver(verbose=False, options={"gap_check": 50})
    with pytest.raises(RuntimeError, match="gap_check needs trace bounds"):
        s.init_problem(p)
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.set_trace_bounds(fx.R[:-1])
    with pytest.raises(RuntimeError, match="trace bounds were set"):
        s.init_problem(p)
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(p)
    with pytest.raises(RuntimeError, match="no trace bounds"):
        s.lower_bound()
    with pytest.raises(RuntimeError, match="bounds for a problem of"):
        s.set_trace_bounds(fx.R[:-1])
    with pytest.raises(RuntimeError, match="gap_check is set before init"):
        s.set_option("gap_check", 50)
    s.set_trace_bounds(fx.R)                                       # after init: allowed
    assert np.isfinite(s.lower_bound()["lower_bound"])
    # behind a failed cuadmm_update_A the bound would come from half-updated matrices: refused, as evaluate() and lambda_min("dual") are
    s.set_XyS(y=np.random.default_rng(6).standard_normal(fx.m))
    s.set_option("update_A_inject_fail", 1)                        # the test hook of tests/test_gpu_update_a.py
    with pytest.raises(cuadmm_amd.CuadmmError) as e:
        s.update_A(p.At_csc_vals * 1.5)
    assert e.value.code == -4
    with pytest.raises(cuadmm_amd.CuadmmError, match=r"lower_bound: the last cuadmm_update_A could not factor the new A A\^T; "
                                                     "the solver needs a successful cuadmm_update_A first") as e:
        s.lower_bound()
    assert e.value.code == -4
    s.update_A(p.At_csc_vals)                                      # a good update on the same handle: the bound is back
    got = s.lower_bound(per_block=True)
    y = s.y
    _against_twin(fx, got, dict(lower_bound(fx, y, fx.R), y=y), fx.R, "B behind a failed and a good update_A")


# ---- 8. command line ------------------------------------------------------------------------------------------------------
def _write_maxcut_dir(d, n, seed):
    """max-cut of a random graph: min <-L/4, X>, X_ii = 1"""
    rng = np.random.default_rng(seed)
    W = np.triu((rng.random((n, n)) < 0.3) * rng.integers(1, 4, size=(n, n)), 1)
    W = W + W.T
    Lap = np.diag(W.sum(1)) - W
    os.makedirs(d)
    with open(d + "blk.txt", "w") as f:
        f.write("s %d\n" % n)
    with open(d + "con_num.txt", "w") as f:
        f.write("%d\n" % n)
    with open(d + "At.txt", "w") as f:
        for i in range(n):
            f.write("%d %d 1\n" % (i * (i + 1) // 2 + i, i))
    with open(d + "b.txt", "w") as f:
        for i in range(n):
            f.write("%d 0 1\n" % i)
    with open(d + "C.txt", "w") as f:
        for i in range(n):
            for j in range(i + 1):
                if Lap[i, j] != 0:
                    f.write("%d 0 %.17g\n" % (i * (i + 1) // 2 + j, -0.25 * Lap[i, j] * (1.0 if i == j else np.sqrt(2.0))))


def test_cli_lower_bound(tmp_path):
    d = str(tmp_path / "maxcut") + "/"
    _write_maxcut_dir(d, 30, 3)
    exe = os.path.join(ROOT, "cuadmm_amd", "lib", "cuadmm_exe")
    js, js0 = str(tmp_path / "with.json"), str(tmp_path / "without.json")
    r = subprocess.run([exe, d, "--trace-bounds=auto", "--gap=50", "--quiet", "--json=" + js], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(js) as f:
        side = json.load(f)
    print({k: side[k] for k in ("status", "iterations", "pobj", "lower_bound", "certified_gap")}, side.get("gap_check"))
    assert math.isfinite(side["lower_bound"]) and side["lower_bound"] <= side["pobj"] + abs(side["pobj"]) * 1e-3
    assert side["status"] in ("converged", "certified_gap") and side["certified_gap"] >= 0
    assert side["lower_bound_parts"]["worst_block"] == 0
    r = subprocess.run([exe, d, "--quiet", "--json=" + js0], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(js0) as f:
        plain = json.load(f)
    assert not {"lower_bound", "certified_gap", "lower_bound_parts", "gap_check"} & set(plain) and plain["status"] == "converged"
    assert set(side) - set(plain) <= {"lower_bound", "certified_gap", "lower_bound_parts", "gap_check"}
    r = subprocess.run([exe, d, "--gap=50", "--quiet"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "trace bounds" in r.stderr
