"""cuadmm_update_A: new values of A on the pattern of a factored solver (include/cuadmm_amd.h; csrc/engine_update.hip, the value pass in
csrc/vec_kernels.hip, the host refactorisation in csrc/aat_ldlt.cpp).  The contract is "the state cuadmm_init with the new values and
the current iterate would have left", and the engine is bit-reproducible, so the check is array_equal against a fresh init.

New values: every nonzero scaled by 1 + 0.05 cos(i), i its position in the caller's value array (the scaling of
tests/_update_bc_common.py: perturb, without its dropped and added entries: the pattern must stay)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd.synthetic import config_c4_blk, make_synthetic
from oracle import cuadmm_oracle as orc
from tests._update_bc_common import INFO, init_with, perturb, snapshot, thin
from tests.conftest import ROOT, load_npz_problem
from tests.helpers import problem_to_amd

pytestmark = pytest.mark.gpu

K1, K2 = 12, 25
SGS, ADMM = 11000, 0
_cache = {}


def problem(name, problem_dirs=None):
    if name not in _cache:
        if name == "closed":
            q = make_synthetic([32] * 300, cons_per_block=5, seed=3, dense_C=False)
        elif name == "mixed":
            q = make_synthetic(config_c4_blk(600, seed=4), cons_per_block=3, seed=4, dense_C=False)
        elif name == "ublock":
            from tests.test_f4_free_and_rank import _problem_with_free_block
            a = _problem_with_free_block()
            _cache[name] = (a, thin(a.b_indices, a.b_vals), thin(a.C_indices, a.C_vals))
            return _cache[name]
        else:
            a = problem_to_amd(orc.load_problem_txt(problem_dirs[name]) if problem_dirs and name in problem_dirs else load_npz_problem(name))
            _cache[name] = (a, (a.b_indices, a.b_vals), (a.C_indices, a.C_vals))
            return _cache[name]
        a = cuadmm_amd.Problem(q.vec_len, q.con_num, q.blk, q.At_col_ptrs, q.At_row_ids, q.At_vals, q.b_idx, q.b_vals, q.C_idx, q.C_vals)
        _cache[name] = (a, thin(a.b_indices, a.b_vals), (a.C_indices, a.C_vals))
    return _cache[name]


def new_vals(a, phase=0.0):
    v = np.asarray(a.At_csc_vals, np.float64)
    return v * (1.0 + 0.05 * np.cos(np.arange(v.size, dtype=np.float64) + phase))


def init_vals(s, a, vals, b, Cv, X0=None, y0=None, S0=None, sig=1.0):
    return s.init(15, 30, a.vec_len, a.con_num, a.At_csc_col_ptrs, a.At_csc_row_ids, vals, a.At_nnz, b[0], b[1], len(b[0]),
                  Cv[0], Cv[1], len(Cv[0]), a.blk_vals, a.mat_num, X0, y0, S0, sig)


def solver(options=None):
    return cuadmm_amd.SDPSolver(verbose=False, options=options)


def solve(s, iters, sw):
    return s.solve(iters, 0.0, 0, 50, 100, sw, 1.05)


def assert_same(u, f, what):
    names = list(INFO) + ["state", "info_iter_num", "X", "y", "S"]
    for nm, va, vb in zip(names, snapshot(u), snapshot(f)):
        assert va.shape == vb.shape and np.array_equal(va, vb), "%s: %s differs (max |d| = %.3e)" % (
            what, nm, float(np.max(np.abs(va - vb))) if va.shape == vb.shape and va.size else -1.0)


def updated_and_fresh(name, sw, keep=True, options=None, problem_dirs=None, read_first=True):
    """U: init, K1 iterations, update_A.  F: a fresh init on the new values from U's iterate (read through U's getters first, or --
    read_first = False -- from a twin, so that U is updated straight from the lazily-unscaled state its solve left)."""
    a, b, Cv = problem(name, problem_dirs)
    v2 = new_vals(a)
    u = solver(options)
    init_with(u, a, b, Cv)
    solve(u, K1, sw)
    src = u
    if not read_first:
        src = solver(options)
        init_with(src, a, b, Cv)
        solve(src, K1, sw)
    sig = src.state()["sig"]
    X0, y0, S0 = (src.X, src.y, src.S) if keep else (None, None, None)
    u.update_A(v2, keep, sig)
    f = solver(options)
    init_vals(f, a, v2, b, Cv, X0, y0, S0, sig)
    return u, f


CASES = [("closed", None), ("mixed", None), ("ublock", None), ("hinf12", None), ("pendulum_N=80", None), ("pendulum_N=80", {"host_solve": 1}),
         ("pendulum_N=80", {"fuse": 0}), ("pendulum_N=80", {"lead_tops": 0}), ("pendulum_N=80", {"tail_k": 1024})]


@pytest.mark.parametrize("name,options", CASES, ids=[n + ("" if o is None else "-" + "-".join("%s=%s" % kv for kv in o.items())) for n, o in CASES])
def test_update_equals_fresh_init(name, options, problem_dirs):
    u, f = updated_and_fresh(name, SGS, options=options, problem_dirs=problem_dirs)
    assert_same(u, f, "after the update")
    assert u.info_iter_num == 0 and u.info_arr("pobj").size == 0 and u.total_time == 0.0
    solve(u, K2, SGS); solve(f, K2, SGS)                  # solve(25, 0, ...)
    assert_same(u, f, "after %d iterations" % K2)
    info = u.update_info()
    assert info[0] == 1 and info[4] == 1 and info[1] > 0 and info[5] >= 8 * problem(name, problem_dirs)[0].At_nnz


@pytest.mark.parametrize("sw", [SGS, ADMM], ids=["sGS", "ADMM"])
@pytest.mark.parametrize("keep", [True, False], ids=["warm", "cold"])
@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_both_phases_warm_and_cold(name, keep, sw):
    u, f = updated_and_fresh(name, sw, keep=keep)
    assert_same(u, f, "after the update")
    solve(u, K2, sw); solve(f, K2, sw)
    assert_same(u, f, "after %d iterations" % K2)


@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_pending_lazily_unscaled_iterate(name):
    u, f = updated_and_fresh(name, SGS, read_first=False)
    solve(u, K2, SGS); solve(f, K2, SGS)
    assert_same(u, f, "updated from the scaled state")


@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_two_updates_in_a_row_and_the_ordering_runs_once(name):
    a, b, Cv = problem(name)
    u = solver()
    init_with(u, a, b, Cv)
    solve(u, K1, SGS)
    u.update_A(new_vals(a), True)
    solve(u, 5, SGS)
    X0, y0, S0, sig = u.X, u.y, u.S, u.state()["sig"]
    v3 = new_vals(a, 1.0)
    u.update_A(v3, True)
    f = solver()
    init_vals(f, a, v3, b, Cv, X0, y0, S0, sig)
    assert_same(u, f, "after the second update")
    solve(u, K2, SGS); solve(f, K2, SGS)
    assert_same(u, f, "second update, %d iterations" % K2)
    u.update_A(np.asarray(a.At_csc_vals, np.float64), False)
    info = u.update_info()
    assert info[0] == 3 and info[4] == 1
    g = solver()
    init_with(g, a, b, Cv, None, None, None, u.state()["sig"])
    solve(u, K2, SGS); solve(g, K2, SGS)
    assert_same(u, g, "back on the original values, cold")


@pytest.mark.parametrize("order", ["A_then_bC", "bC_then_A"])
@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_update_A_and_update_bC(name, order):
    a, b, Cv = problem(name)
    b2, C2 = perturb(b[0], b[1], a.con_num), perturb(Cv[0], Cv[1], a.vec_len)
    v2 = new_vals(a)
    u = solver()
    init_with(u, a, b, Cv)
    solve(u, K1, SGS)
    # (an update takes the iterate as it stands, like init its X0: a solve between the two puts it back into the caller's units)
    if order == "A_then_bC":
        u.update_A(v2, True)
        solve(u, 5, SGS)
        X0, y0, S0, sig = u.X, u.y, u.S, u.state()["sig"]
        u.update_bC(b2[0], b2[1], C2[0], C2[1], True)
    else:
        u.update_bC(b2[0], b2[1], C2[0], C2[1], True)
        solve(u, 5, SGS)
        X0, y0, S0, sig = u.X, u.y, u.S, u.state()["sig"]
        u.update_A(v2, True)
    f = solver()
    init_vals(f, a, v2, b2, C2, X0, y0, S0, sig)
    solve(u, K2, SGS); solve(f, K2, SGS)
    assert_same(u, f, order)


@pytest.mark.parametrize("order", ["A_then_bC", "bC_then_A"])
@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_update_A_and_update_bC_back_to_back(name, order):
    """No solve between the two calls (what cuadmm_exe --then-A= runs).  The second update takes the iterate as the first left it, as
    init takes its X0: read from a twin that made the same first update, so that U itself goes from one update into the other with
    y still on the device only where the first left it there."""
    a, b, Cv = problem(name)
    b2, C2 = perturb(b[0], b[1], a.con_num), perturb(Cv[0], Cv[1], a.vec_len)
    v2 = new_vals(a)
    u, t = solver(), solver()
    for s in (u, t):
        init_with(s, a, b, Cv)
        solve(s, K1, SGS)
        if order == "A_then_bC":
            s.update_A(v2, True)
        else:
            s.update_bC(b2[0], b2[1], C2[0], C2[1], True)
    X0, y0, S0, sig = t.X, t.y, t.S, t.state()["sig"]
    if order == "A_then_bC":
        u.update_bC(b2[0], b2[1], C2[0], C2[1], True)
    else:
        u.update_A(v2, True)
    f = solver()
    init_vals(f, a, v2, b2, C2, X0, y0, S0, sig)
    assert_same(u, f, order + " after the second update")
    solve(u, K2, SGS); solve(f, K2, SGS)
    assert_same(u, f, order)


@pytest.mark.parametrize("where", [1, 2], ids=["behind_host_factor", "behind_device_rebuild"])
@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_failed_update_refuses_solve_and_a_good_update_recovers(name, where):
    """The engine's path behind a factorisation that broke down, through the test hook update_A_inject_fail (no finite
    values were found for which init's factorisation of A A^T + 1e-15 I fails, so the failure is injected behind the host
    refactorisation, or behind the rebuilt GPU tail and y-solve streams): CUADMM_ERR_FACTOR, solve and update_bC refuse with it,
    X / y / S stay readable in the caller's units, and a good update_A leaves the state a fresh init leaves."""
    a, b, Cv = problem(name)
    v2 = new_vals(a)
    u = solver()
    init_with(u, a, b, Cv)
    solve(u, K1, SGS)
    X0, y0, S0, sig = u.X, u.y, u.S, u.state()["sig"]
    u.set_option("update_A_inject_fail", where)
    with pytest.raises(cuadmm_amd.CuadmmError) as e:
        u.update_A(new_vals(a, 2.0))
    assert e.value.code == -4
    for call in (lambda: solve(u, 3, SGS), lambda: u.update_bC(b[0], b[1])):
        with pytest.raises(cuadmm_amd.CuadmmError) as e:
            call()
        assert e.value.code == -4 and "update_A" in str(e.value)
    assert np.array_equal(u.X, X0) and np.array_equal(u.y, y0) and np.array_equal(u.S, S0)
    u.update_A(v2, True)
    f = solver()
    init_vals(f, a, v2, b, Cv, X0, y0, S0, sig)
    assert_same(u, f, "recovered")
    solve(u, K2, SGS); solve(f, K2, SGS)
    assert_same(u, f, "recovered, %d iterations" % K2)


def test_accel_memory_starts_empty():
    u, f = updated_and_fresh("pendulum_N=80", ADMM, options={"accel": 5})
    solve(u, K2, ADMM); solve(f, K2, ADMM)
    assert_same(u, f, "accel = 5")


def test_refusals_leave_the_solver_as_it_was():
    a, b, Cv = problem("closed")
    u, r = solver(), solver()
    for s in (u, r):
        init_with(s, a, b, Cv)
        solve(s, K1, SGS)
    good = new_vals(a)
    for bad, word in ((good[:-1], "values"), (np.concatenate([good, [1.0]]), "values"), (np.where(np.arange(good.size) == 7, np.nan, good), "finite"),
                      (np.where(np.arange(good.size) == good.size - 1, np.inf, good), "finite")):
        with pytest.raises(cuadmm_amd.CuadmmError) as e:
            u.update_A(bad)
        assert e.value.code == -1 and word in str(e.value)
    assert u.update_info()[0] == 0
    u.solve(K2, 0.0, 0, 50, 100, SGS, 1.05, if_first=False); r.solve(K2, 0.0, 0, 50, 100, SGS, 1.05, if_first=False)
    assert_same(u, r, "after the refused calls")


def test_explicit_zero_is_accepted_as_init_keeps_it():
    """init drops nothing from the pattern, so a value of exactly 0 is as good as any other: same bits as a fresh init with it"""
    a, b, Cv = problem("closed")
    v2 = new_vals(a)
    v2[3] = 0.0
    u = solver()
    init_with(u, a, b, Cv)
    solve(u, K1, SGS)
    X0, y0, S0, sig = u.X, u.y, u.S, u.state()["sig"]
    u.update_A(v2, True)
    f = solver()
    init_vals(f, a, v2, b, Cv, X0, y0, S0, sig)
    solve(u, K2, SGS); solve(f, K2, SGS)
    assert_same(u, f, "explicit zero")


@pytest.mark.parametrize("name", ["duo", "pendulum_N=80"])
def test_in_process_group_forwards_the_update(name):
    """duo_init(device_num_requested = 2, duo_share_device = 1) on a block-diagonal input with two sizes (owned constraints: every rank
    refactors its own A A^T, the norms of all constraints from the full values) and on pendulum N = 80 (coupled: the replicated y-solve,
    the tail's rows kept per rank), update through the leader; against a fresh group at the tolerance tests/test_gpu_update_bc.py and
    tests/test_gpu_solver.py use between two groups / a group and a single engine (1e-9 / 1e-12: a group's exchange is not bit-ordered)."""
    from tests.test_gpu_solver import _cmp
    if name == "duo":
        q = make_synthetic([12] * 40 + [30] * 24, cons_per_block=4, seed=6, dense_C=False)
        a = cuadmm_amd.Problem(q.vec_len, q.con_num, q.blk, q.At_col_ptrs, q.At_row_ids, q.At_vals, q.b_idx, q.b_vals, q.C_idx, q.C_vals)
        b, Cv = thin(a.b_indices, a.b_vals), (a.C_indices, a.C_vals)
    else:
        a, b, Cv = problem(name)
    v2 = new_vals(a)

    def duo(vals, X0=None, y0=None, S0=None, sig=1.0):
        s = solver({"duo_share_device": 1})
        s.duo_init(True, 2, 15, 30, a.vec_len, a.con_num, a.At_csc_col_ptrs, a.At_csc_row_ids, vals, a.At_nnz, b[0], b[1], len(b[0]),
                   Cv[0], Cv[1], len(Cv[0]), a.blk_vals, a.mat_num, X0, y0, S0, sig)
        return s
    u = duo(a.At_csc_vals)
    solve(u, K1, SGS)
    assert u.group_info()["engines"] == 2
    X0, y0, S0, sig = u.X, u.y, u.S, u.state()["sig"]
    u.update_A(v2, True, sig)
    f = duo(v2, X0, y0, S0, sig)
    solve(u, K2, SGS); solve(f, K2, SGS)
    assert u.info_iter_num == f.info_iter_num == K2 and u.info_arr("pobj").size == K2
    for nm in ("errRp", "errRd", "pobj", "dobj", "relgap"):
        _cmp("group:" + nm, u.info_arr(nm), f.info_arr(nm), rtol=1e-9, atol=1e-12)
    assert np.array_equal(u.info_arr("sig"), f.info_arr("sig"))
    assert np.array_equal(u.info_arr("bscale"), f.info_arr("bscale"))
    for va, vb in ((u.X, f.X), (u.y, f.y), (u.S, f.S)):
        assert va.shape == vb.shape and np.max(np.abs(va - vb)) <= 1e-9 * (1 + np.max(np.abs(vb)))
    with pytest.raises(cuadmm_amd.CuadmmError):                # refused by the leader before any rank sees it
        u.update_A(v2[:-1])


# ---- the command line ------------------------------------------------------------------------------------------------------
def _cli_dirs(tmp_path, problem_dirs):
    import shutil
    d1 = str(tmp_path / "stage1") + "/"                         # copies: the session's directory stays without an X_opt.txt
    d2 = str(tmp_path / "stage2") + "/"
    shutil.copytree(problem_dirs["hinf12"], d1)
    shutil.copytree(problem_dirs["hinf12"], d2)
    for fn in ("X_opt.txt",):
        if os.path.exists(d2 + fn):
            os.remove(d2 + fn)
    rows = [ln.split() for ln in open(d1 + "At.txt") if ln.strip()]
    with open(d2 + "At.txt", "w") as f:
        for i, (r, c, v) in enumerate(rows):
            f.write("%s %s %.17g\n" % (r, c, float(v) * (1.0 + 0.05 * np.cos(float(i)))))
    return d1, d2


def test_cli_then_A_equals_the_library_sequence(tmp_path, problem_dirs):
    """cuadmm_exe dir/ --then-A=dir2/: dir2's values of A on the same pattern, then its b and C, warm start; dir2/X_opt.txt against the
    same sequence through the Python wrapper (the file holds 32 decimals)"""
    d1, d2 = _cli_dirs(tmp_path, problem_dirs)
    exe = os.path.join(ROOT, "cuadmm_amd", "lib", "cuadmm_exe")
    r = subprocess.run([exe, d1, "--then-A=" + d2, "--quiet", "--max_iter=40"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.loadtxt(d2 + "X_opt.txt")
    p1, p2 = problem_to_amd(orc.load_problem_txt(d1)), problem_to_amd(orc.load_problem_txt(d2))
    assert np.array_equal(p1.At_csc_row_ids, p2.At_csc_row_ids) and not np.array_equal(p1.At_csc_vals, p2.At_csc_vals)
    s = solver()
    init_with(s, p1, (p1.b_indices, p1.b_vals), (p1.C_indices, p1.C_vals))
    s.solve(40, 1e-3, 0, 50, 100, 5000, 1.05)
    s.update_A(p2.At_csc_vals, True)
    s.update_bC(p2.b_indices, p2.b_vals, p2.C_indices, p2.C_vals, True)
    s.solve(40, 1e-3, 0, 50, 100, 5000, 1.05)
    assert got.shape == s.X.shape and np.max(np.abs(got - s.X)) <= 1e-31


def test_cli_then_A_refuses_another_pattern(tmp_path, problem_dirs):
    d1, d2 = _cli_dirs(tmp_path, problem_dirs)
    rows = open(d2 + "At.txt").read().splitlines()
    open(d2 + "At.txt", "w").write("\n".join(rows[:-1]) + "\n")          # one entry fewer
    exe = os.path.join(ROOT, "cuadmm_amd", "lib", "cuadmm_exe")
    r = subprocess.run([exe, d1, "--then-A=" + d2, "--quiet", "--max_iter=5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--then-A" in r.stderr and "pattern" in r.stderr
    assert not os.path.exists(d2 + "X_opt.txt")


def test_the_two_passes_are_timed_alone_under_option_profile():
    a, b, Cv = problem("closed")
    for prof in (0, 1):
        s = cuadmm_amd.SDPSolver(verbose=False, profile=prof)
        init_with(s, a, b, Cv)
        solve(s, K1, SGS)
        s.update_A(new_vals(a), True)
        ms_v, by_v, ms_s, by_s = s.update_pass_info()
        assert by_v == 20.0 * 2 * a.At_nnz and by_s == 32.0 * a.vec_len          # every entry once in A, once in A^T; X and S read and written
        assert (ms_v > 0 and ms_s > 0) if prof else (ms_v == 0 and ms_s == 0)


@pytest.mark.parametrize("n", [1, 3, 257, 64 * 1024 + 5])
@pytest.mark.parametrize("offA,offAt", [(0, 0), (1, 0), (0, 1), (3, 5)])
def test_value_pass_against_numpy(n, offA, offAt):
    """gather_vals_kernel: both targets from one source through their maps; targets that start on and off a 16-byte boundary, odd and
    even lengths, more than one workgroup; nothing outside the targets is written"""
    lib = cuadmm_amd.load()
    rng = np.random.default_rng(n + 7 * offA + offAt)
    src = rng.standard_normal(n)
    nA, nAt = n, max(1, n - 2)
    fA = rng.permutation(n).astype(np.int32)
    fAt = rng.integers(0, n, nAt).astype(np.int32)
    outA, outAt = np.empty(nA + offA + 2), np.empty(nAt + offAt + 2)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.cuadmm_op_gather_vals(P(src), n, P(fA), nA, offA, P(fAt), nAt, offAt, -7.5, P(outA), P(outAt)) == 0
    refA, refAt = np.full(nA + offA + 2, -7.5), np.full(nAt + offAt + 2, -7.5)
    refA[offA:offA + nA] = src[fA]
    refAt[offAt:offAt + nAt] = src[fAt]
    assert np.array_equal(outA, refA) and np.array_equal(outAt, refAt)
