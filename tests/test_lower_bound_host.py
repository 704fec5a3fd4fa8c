"""The certified lower bound without a device: the trace-bound detection (cuadmm_trace_bounds_detect), the validation of the option
and of cuadmm_set_trace_bounds, and the numpy twin on its own fixtures (include/cuadmm_amd.h; csrc/lower_bound.hip;
tests/_lower_bound_twin.py).

tests/golden/ holds a theta-function input (1dc.1024: one block, tr X = 1) and no max-cut input; the max-cut shape (every diagonal
entry fixed to 1, R = n) is hand-made here.
"""
import ctypes as C

import numpy as np
import pytest

import cuadmm_amd
from tests._lower_bound_twin import lb_tolerance, lower_bound, make_opt_fixture, twin_solve
from tests.conftest import load_npz_problem
from tests.helpers import problem_to_amd

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def diag_slot(i):
    return i * (i + 1) // 2 + i


def problem(blk, rows, b):
    """rows: list of {svec slot: value}"""
    r, c, v = [], [], []
    for j, row in enumerate(rows):
        for slot, val in row.items():
            r.append(slot); c.append(j); v.append(val)
    bi = np.nonzero(np.asarray(b))[0]
    return cuadmm_amd.Problem.from_coo(blk, len(rows), np.array(r), np.array(c), np.array(v, np.float64), bi, np.asarray(b, np.float64)[bi],
                                       np.zeros(0, np.int32), np.zeros(0))


def offsets(blk):
    lens = [n * (n + 1) // 2 if n > 0 else -n for n in blk]
    return np.concatenate([[0], np.cumsum(lens)])


def identity_row(off, n, c):
    return {int(off + diag_slot(i)): c for i in range(n)}


def test_detect_both_rules_and_what_gives_no_bound():
    blk = [3, 4, -2, 2, 5, 3, 1]
    off = offsets(blk)
    rows, b = [], []
    rows.append(identity_row(off[0], 3, 2.5)); b.append(5.0)                        # block 0: rule 1 with a scaled identity, tr = 2
    for i in range(4):                                                              # block 1: rule 2, diagonal entries 1, 2, 3, 4
        rows.append({int(off[1] + diag_slot(i)): 2.0}); b.append(2.0 * (i + 1))
    rows.append({int(off[2]): 1.0}); b.append(1.0)                                  # the unconstrained block: never a bound
    rows.append({**identity_row(off[3], 2, 1.0), int(off[4]): 1.0}); b.append(1.0)      # touches blocks 3 and 4: no bound
    for i in range(4):                                                              # block 4: only four of five diagonal entries fixed
        rows.append({int(off[4] + diag_slot(i)): 1.0}); b.append(1.0)
    rows.append(identity_row(off[5], 3, 1.0)); b.append(-1.0)                       # block 5: a negative right-hand side
    rows.append({int(off[6]): 4.0}); b.append(2.0)                                  # block 6 (n = 1): both rules see the row, 0.5
    rows.append({int(off[0] + 1): 1.0}); b.append(0.3)                              # an off-diagonal entry fixed: nothing
    R = problem(blk, rows, b).trace_bounds()
    assert R.tolist() == [2.0, 10.0, -1.0, -1.0, -1.0, -1.0, 0.5]


def test_detect_takes_the_smaller_bound_and_skips_negative_entries():
    blk = [3, 2]
    off = offsets(blk)
    rows, b = [], []
    rows.append(identity_row(off[0], 3, 1.0)); b.append(7.0)                        # rule 1: 7
    for i in range(3):
        rows.append({int(off[0] + diag_slot(i)): 1.0}); b.append(2.0)               # rule 2: 6
    rows.append({int(off[1] + diag_slot(0)): 1.0}); b.append(1.0)
    rows.append({int(off[1] + diag_slot(1)): 1.0}); b.append(-1.0)                  # a negative diagonal entry: rule 2 finds nothing
    rows.append(identity_row(off[1], 2, -2.0)); b.append(-6.0)                      # rule 1 with c = -2: tr = 3
    assert problem(blk, rows, b).trace_bounds().tolist() == [6.0, 3.0]
    # the max-cut shape: every diagonal entry 1
    n = 17
    R = problem([n], [{diag_slot(i): 1.0} for i in range(n)], [1.0] * n).trace_bounds()
    assert R.tolist() == [float(n)]


def test_detect_on_the_golden_theta_input():
    p = problem_to_amd(load_npz_problem("1dc.1024"))
    assert p.trace_bounds().tolist() == [1.0]


def test_detect_refuses_blocks_that_do_not_cover_the_vector():
    lib = cuadmm_amd.load()
    cp, blk, R = np.zeros(2, np.int32), np.array([3], np.int32), np.zeros(1)
    assert lib.cuadmm_trace_bounds_detect(7, 1, P(cp), None, None, None, None, 0, P(blk), 1, P(R)) == -1
    assert "vec_len" in lib.cuadmm_last_error().decode()


def test_option_and_bounds_validation():
    s = cuadmm_amd.SDPSolver(verbose=False)
    for bad in (1, -3, 2.5, 1e6 + 1, float("nan")):
        with pytest.raises(RuntimeError, match="gap_check"):
            s.set_option("gap_check", bad)
    with pytest.raises(RuntimeError, match="gap_tol"):
        s.set_option("gap_tol", -1e-3)
    for ok in (0, 2, 50, 1e6):
        s.set_option("gap_check", ok)
    s.set_option("gap_check", 0)
    s.set_trace_bounds([1.0, 2.0, 0.0])
    for bad in ([1.0, -1e-300, 2.0], [1.0, float("nan"), 2.0], [float("inf"), 1.0, 1.0]):
        with pytest.raises(RuntimeError, match="finite and not negative"):
            s.set_trace_bounds(bad)
    lib = cuadmm_amd.load()
    assert lib.cuadmm_set_trace_bounds(s._h, P(np.ones(3)), 0) == -1
    s.set_trace_bounds(None)                                     # clears
    s.set_trace_bounds([3.0])
    for q in (s.gap_info(), s.status()):
        assert q["checks"] == 0
    assert s.status()["name"] == "none" and cuadmm_amd.SDPSolver.STATUS_NAMES[5] == "certified_gap"
    with pytest.raises(RuntimeError, match="not initialised"):
        s.lower_bound()


def test_twin_bound_is_valid_and_tight_at_the_optimum():
    for blk, m in (([3, 20, 70, -2, 130], 40), ([1] * 40 + [2, 5, 8, -3, 33], 30)):
        fx = make_opt_fixture(blk, m, 1)
        assert abs(float(fx.C @ fx.Xs) - fx.pstar) <= 1e-12 * (1 + abs(fx.pstar)) and np.allclose(fx.A @ fx.Xs, fx.b)
        at = lower_bound(fx, fx.ys, fx.R)
        far = lower_bound(fx, np.random.default_rng(5).standard_normal(fx.m), fx.R)
        print(blk[-1], "p* %.12g, LB(y*) %.12g, LB(random y) %.6g" % (fx.pstar, at["lb"], far["lb"]))
        assert far["lb"] <= at["lb"] <= fx.pstar
        assert fx.pstar - at["lb"] <= float(np.sum(fx.R * (at["nubar"] - at["nu"]))) + lb_tolerance(fx, at, fx.R)


def test_twin_rule_ends_a_solve_with_status_5():
    fx = make_opt_fixture([1] * 40 + [2, 5, 8, -3, 33], 30, 1)
    r = twin_solve(fx, fx.R, 50, 1e-3, 3000, 1e-6)
    assert r.status == 5 and r.iteration % 50 == 0 and r.checks[-1][2] <= 1e-3 < r.checks[-2][2]
    assert all(lb <= fx.pstar for _, lb, _, _ in r.checks)
