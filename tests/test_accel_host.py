"""Option "accel" without a device: the numpy twin against the oracle it is built on, the host least-squares solve, the option's
range (include/cuadmm_amd.h; csrc/accel.hip: accel_solve_ls; tests/_accel_twin.py)."""
import ctypes as C

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd.synthetic import make_synthetic
from oracle import cuadmm_oracle as orc
from tests._accel_twin import accel_solve
from tests.test_gpu_moment_parity import load_problem

NAMES = ("pobj", "dobj", "errRp", "errRd", "relgap", "sig")


def _synthetic():
    q = make_synthetic([5, 12, 20, 7], cons_per_block=3, seed=11)
    return orc.Problem(q.vec_len, q.con_num, q.blk, q.At_col_ptrs, q.At_row_ids, q.At_vals, q.b_idx, q.b_vals, q.C_idx, q.C_vals)


@pytest.mark.parametrize("name", ["hinf12", "synthetic"])
def test_twin_without_acceleration_is_the_oracle(name, tmp_path):
    """30 iterations, sGS until iteration 10, then ADMM with the best-iterate bookkeeping: bit for bit"""
    p = _synthetic() if name == "synthetic" else load_problem(name, tmp_path)
    a, b = orc.OracleSolver().init_problem(p), orc.OracleSolver().init_problem(p)
    ia = a.solve(30, 0.0, 0, 50, 100, 10, 1.05)
    ib, log = accel_solve(b, 30, 0.0, 0, 50, 100, 10, 1.05, accel=0)
    assert ia.iter_num == ib.iter_num == 30 and log.taken == 0
    for nm in NAMES:
        assert np.array_equal(np.array(getattr(ia, nm)), np.array(getattr(ib, nm))), nm
    assert np.array_equal(a.X, b.X) and np.array_equal(a.y, b.y) and np.array_equal(a.S, b.S)
    assert ia.log_rows == ib.log_rows and ia.final_msg == ib.final_msg


def _ld_solve(M, r):
    """Gaussian elimination with partial pivoting in longdouble (numpy.linalg has no longdouble path)"""
    M, r = M.astype(np.longdouble).copy(), r.astype(np.longdouble).copy()
    n = r.size
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        M[[k, p]], r[[k, p]] = M[[p, k]], r[[p, k]]
        for i in range(k + 1, n):
            f = M[i, k] / M[k, k]
            M[i, k:] -= f * M[k, k:]
            r[i] -= f * r[k]
    x = np.zeros(n, np.longdouble)
    for i in range(n - 1, -1, -1):
        x[i] = (r[i] - np.dot(M[i, i + 1:], x[i + 1:])) / M[i, i]
    return x


def _ls_case(cols, near_equal):
    rng = np.random.default_rng(100 + cols)
    D = rng.standard_normal((cols, 400))
    if near_equal:       # two nearly equal columns: cond(G) ~ (|d| / |d0 - d1|)^2 ~ 1e12 before the regularisation
        D[1] = D[0] + 1e-6 * rng.standard_normal(400)
    G = D @ D.T
    return G, D @ rng.standard_normal(400)


@pytest.mark.parametrize("cols,near_equal", [(1, False), (2, False), (7, False), (16, False), (7, True)])
def test_solve_ls_against_longdouble(cols, near_equal):
    """Tolerance: a Cholesky solve in precision u_ld has forward error <= c n cond(M) u_ld (Higham, ASNA Th. 10.4 with c n ~ 4 n^2
    for the two triangular solves and the factor); the same bound holds for the longdouble elimination it is compared with; plus
    the rounding of gamma to double."""
    lib = cuadmm_amd.load()
    G, rhs = _ls_case(cols, near_equal)
    reg = 1e-10
    if near_equal:
        assert np.linalg.cond(G) > 1e11
    M = G.astype(np.longdouble) + np.longdouble(reg) * np.trace(G.astype(np.longdouble)) / cols * np.eye(cols, dtype=np.longdouble)
    ref = _ld_solve(M, rhs)
    out = np.zeros(cols)
    Gc, rc_ = np.ascontiguousarray(G), np.ascontiguousarray(rhs)
    rc = lib.cuadmm_accel_solve_ls(Gc.ctypes.data_as(C.c_void_p), rc_.ctypes.data_as(C.c_void_p), cols, reg, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.cuadmm_last_error()
    cond = float(np.linalg.cond(M.astype(np.float64)))
    tol = 2 * 4 * cols * cols * cond * float(np.finfo(np.longdouble).eps) + 2 * np.finfo(np.float64).eps
    err = float(np.max(np.abs(out - ref)) / np.max(np.abs(ref)))
    print("cols %d cond %.2e: error %.2e (bound %.2e)" % (cols, cond, err, tol))
    assert err <= tol
    # a matrix that is not positive definite is reported, not solved
    bad = -np.eye(cols)
    assert lib.cuadmm_accel_solve_ls(bad.ctypes.data_as(C.c_void_p), rc_.ctypes.data_as(C.c_void_p), cols, 0.0, out.ctypes.data_as(C.c_void_p)) == -4
    assert lib.cuadmm_accel_solve_ls(Gc.ctypes.data_as(C.c_void_p), rc_.ctypes.data_as(C.c_void_p), 17, reg, out.ctypes.data_as(C.c_void_p)) == -1


def test_option_range():
    lib = cuadmm_amd.load()
    h = C.c_void_p()
    assert lib.cuadmm_create(C.byref(h)) == 0
    try:
        for bad in (17.0, -1.0, 2.5):
            assert lib.cuadmm_set_option(h, b"accel", bad) == -1 and b"accel" in lib.cuadmm_last_error()
        for good in (0.0, 1.0, 16.0):
            assert lib.cuadmm_set_option(h, b"accel", good) == 0
        assert lib.cuadmm_set_option(h, b"accel_safeguard", 0.0) == 0 and lib.cuadmm_set_option(h, b"accel_reg", 1e-8) == 0
        o = np.zeros(8)
        assert lib.cuadmm_get_accel_info(h, o.ctypes.data_as(C.c_void_p)) == 0
        assert o[0] == 16 and not o[1:].any()
    finally:
        lib.cuadmm_destroy(h)


@pytest.mark.parametrize("sw", [0, 11000])
def test_recorded_twin_trajectory_is_the_twin(sw, tmp_path):
    """tests/golden/accel_twin_traj.json (the reference of the GPU trajectory tests) against a fresh twin run, on the small input"""
    import json
    import os
    from tests.conftest import GOLDEN
    from tests.golden.make_accel_traj import ITERS, MEM, NAMES as REC, run
    with open(os.path.join(GOLDEN, "accel_twin_traj.json")) as f:
        rec = json.load(f)["hinf12/%d" % sw]
    got, log = run(load_problem("hinf12", tmp_path), sw, iters=ITERS, mem=MEM)
    for nm in REC:
        assert np.array_equal(np.array(got[nm]), np.array(rec[nm])), nm
    assert [[i, d] for i, d in log.decisions] == rec["decisions"] and log.first_accept == rec["first_accept"]
    assert (log.taken, log.accepted, log.rejected, log.restarts) == (rec["taken"], rec["accepted"], rec["rejected"], rec["restarts"])
    assert log.accepted >= 3 and log.restarts >= 1
