"""Option "accel": safeguarded Anderson acceleration behind the iteration ("Acceleration"; csrc/accel.hip, csrc/engine_iter.hip).

Op level: the three kernels against numpy in longdouble.  Engine level: accel = 0 changes nothing; trajectories against the numpy
twin (tests/_accel_twin.py, recorded in tests/golden/accel_twin_traj.json by tests/golden/make_accel_traj.py); the safeguard drill;
reproducibility; update_bC / continued solves; the refusals; convergence.

Trajectory tolerances.  Up to and including the first accepted candidate: 1e-8 relative (the head tolerance of
tests/test_gpu_moment_parity.py, with its ATOL floors).  Behind it the gamma solve amplifies rounding: 10 x the spread between two
twin runs whose gammas differ by 1 + 1e-13 cos(j), ON TOP OF the deviation the same run shows over its head -- the engine and numpy
do not agree better than that before any gamma is solved, so it is the floor of what the tail can agree to.  Measured
(make_accel_traj.py, 60 iterations, accel = 5; spread ADMM / sGS; then the engine's largest head / tail deviation over the three
option sets):
    hinf12         5.2e-13 / 1.2e-12     ADMM 0 / 7.3e-13, sGS 0 / 1.5e-12          (switch at 10: spread 1.9e-13)
    ublock         1.2e-12 / 3.7e-13     ADMM 0 / 4.8e-13, sGS 0 / 0
    closed         3.4e-15 / 9.7e-14     0 / 0 throughout (under the ATOL floors)     (switch at 10: spread 9.7e-14)
    pendulum_N=80  9.9e-14 / 1.1e-12     ADMM 5.0e-11 / 2.1e-12, sGS 3.4e-12 / 9.0e-13
(pendulum in the ADMM phase is the one case above 10 x spread alone: 2.1e-12 against 9.9e-13, with 5.0e-11 already in its head.)
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd._lib import check
from cuadmm_amd.synthetic import config_c4_blk, make_synthetic
from tests._update_bc_common import INFO, init_with, perturb, snapshot, thin
from tests.conftest import GOLDEN, load_npz_problem
from tests.helpers import problem_to_amd
from tests.test_gpu_moment_parity import rel_dev

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
SGS, ADMM, CROSS = 11000, 0, 10
_cache = {}


def amd_problem(name):
    """the inputs of tests/test_gpu_update_bc.py (local copies of its few lines) -> cuadmm_amd.Problem"""
    if name not in _cache:
        if name == "closed":
            q = make_synthetic([32] * 300, cons_per_block=5, seed=3, dense_C=False)
        elif name == "mixed":
            q = make_synthetic(config_c4_blk(600, seed=4), cons_per_block=3, seed=4, dense_C=False)
        elif name == "ublock":
            from tests.test_f4_free_and_rank import _problem_with_free_block
            _cache[name] = _problem_with_free_block()
            return _cache[name]
        elif os.path.isdir(os.path.join(GOLDEN, "problems", name)):
            import tempfile
            from tests.test_gpu_moment_parity import load_problem
            _cache[name] = problem_to_amd(load_problem(name, tempfile.mkdtemp()))
            return _cache[name]
        else:
            _cache[name] = problem_to_amd(load_npz_problem(name))
            return _cache[name]
        _cache[name] = cuadmm_amd.Problem(q.vec_len, q.con_num, q.blk, q.At_col_ptrs, q.At_row_ids, q.At_vals, q.b_idx, q.b_vals, q.C_idx, q.C_vals)
    return _cache[name]


def solver(options=None, **kw):
    return cuadmm_amd.SDPSolver(verbose=False, options=options, **kw)


def run(name, iters, sw, options=None, tol=0.0):
    s = solver(options)
    s.init_problem(amd_problem(name))
    s.solve(iters, tol, 0, 50, 100, sw, 1.05)
    return s


def ulps(got, ref):
    """|got - ref| in units of the spacing of doubles at ref (ref in longdouble)"""
    r64 = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, LD) - ref) / np.spacing(np.maximum(np.abs(r64), np.finfo(np.float64).tiny)).astype(LD)


# ------------------------------------------------------------------------------------------------------------------- op level
LS = [1, 3, 40, 257, 64 * 1024 + 5]          # 40: less than one wavefront; odd: scalar tail and a misaligned S half


@pytest.mark.parametrize("have_prev", [0, 1])
@pytest.mark.parametrize("L", LS)
def test_op_push(L, have_prev):
    lib = cuadmm_amd.load()
    rng = np.random.default_rng(L + have_prev)
    u, f0, g0 = rng.standard_normal(2 * L), rng.standard_normal(2 * L), rng.standard_normal(2 * L)
    X, S, sig = rng.standard_normal(L), rng.standard_normal(L), 1.7
    f, g = f0.copy(), np.full(2 * L, np.nan)
    dF0, dG0 = rng.standard_normal(2 * L), rng.standard_normal(2 * L)
    dF, dG, n2 = dF0.copy(), dG0.copy(), np.zeros(1)
    check(lib.cuadmm_op_accel_push(L, P(u), P(X), P(S), sig, P(f), P(g0), have_prev, P(g), P(dF), P(dG), P(n2)))
    xs = np.concatenate([X, S])
    sc = np.concatenate([np.ones(L), np.full(L, sig)]).astype(LD)
    assert np.array_equal(f, xs)                                                     # the fallback is a copy
    assert float(np.max(ulps(g, sc * (xs.astype(LD) - u)))) <= 2
    if have_prev:
        assert float(np.max(ulps(dF, sc * (xs.astype(LD) - f0)))) <= 2
        assert float(np.max(ulps(dG, g.astype(LD) - g0))) <= 2                       # from the g the kernel stored
    else:
        assert np.array_equal(dF, dF0) and np.array_equal(dG, dG0)                   # untouched
    ref = np.sum(g.astype(LD) ** 2)
    assert abs(LD(n2[0]) - ref) <= 4 * EPS * ref


@pytest.mark.parametrize("cols", [1, 2, 16])
@pytest.mark.parametrize("L", LS)
def test_op_gram(L, cols):
    lib = cuadmm_amd.load()
    rng = np.random.default_rng(7 * L + cols)
    ring, g = rng.standard_normal((cols, 2 * L)), rng.standard_normal(2 * L)
    newest = cols // 2
    out, out2 = np.zeros(2 * cols), np.zeros(2 * cols)
    check(lib.cuadmm_op_accel_gram(2 * L, cols, newest, P(ring), P(g), P(out)))
    check(lib.cuadmm_op_accel_gram(2 * L, cols, newest, P(ring), P(g), P(out2)))
    assert np.array_equal(out, out2)                                                 # bit-identical between two calls
    rl, gl = ring.astype(LD), g.astype(LD)
    for j in range(cols):
        for got, a, b in ((out[j], rl[newest], rl[j]), (out[cols + j], rl[j], gl)):
            assert abs(LD(got) - np.sum(a * b)) <= 4 * EPS * np.sum(np.abs(a * b)), (j, got)


@pytest.mark.parametrize("cols", [1, 2, 16])
@pytest.mark.parametrize("L", LS)
def test_op_combine(L, cols):
    """inputs as the engine meets them: a correction that is small beside the iterate (|sum gamma dF| <~ 0.1 |f|, |f| >= 0.5), so
    that the longdouble reference itself is good to a few hundredths of an ulp of the result"""
    lib = cuadmm_amd.load()
    rng = np.random.default_rng(13 * L + cols)
    sign = lambda n: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    X, S = sign(L) * (0.5 + rng.random(L)), sign(L) * (0.5 + rng.random(L))
    ring, gamma, sig = 1e-2 * rng.standard_normal((cols, 2 * L)), rng.standard_normal(cols), 0.37
    Xo, So = X.copy(), S.copy()
    check(lib.cuadmm_op_accel_combine(L, cols, P(ring), P(gamma), sig, P(Xo), P(So)))
    corr = gamma.astype(LD) @ ring.astype(LD)
    assert float(np.max(ulps(Xo, X.astype(LD) - corr[:L]))) <= 2
    assert float(np.max(ulps(So, (LD(sig) * S.astype(LD) - corr[L:]) / LD(sig)))) <= 2


# ------------------------------------------------------------------------------------------------------------- off means off
@pytest.mark.parametrize("name", ["closed", "mixed", "pendulum_N=80"])
def test_accel_zero_is_the_plain_engine(name):
    a, b = run(name, 25, ADMM, {"accel": 0}), run(name, 25, ADMM)
    for nm, va, vb in zip(list(INFO) + ["state", "info_iter_num", "X", "y", "S"], snapshot(a), snapshot(b)):
        assert np.array_equal(va, vb), nm
    assert a.accel_info()["taken"] == 0 and a.accel_info()["ring_bytes"] == 0
    if name == "closed":
        assert a.counters()["batch_launches"] > 0 and a.counters() == b.counters()


# ------------------------------------------------------------------------------------------------ trajectory against the twin
def twin(key):
    if "twin" not in _cache:
        with open(os.path.join(GOLDEN, "accel_twin_traj.json")) as f:
            _cache["twin"] = json.load(f)
    return _cache["twin"][key]


@pytest.mark.parametrize("options", [None, {"fuse": 0}, {"host_solve": 1}], ids=["default", "unfused", "host_solve"])
@pytest.mark.parametrize("name,sw", [(n, w) for n in ("pendulum_N=80", "hinf12", "ublock", "closed") for w in (ADMM, SGS)] +
                         [("hinf12", CROSS), ("closed", CROSS)])     # CROSS: restart at the switch, best-iterate bookkeeping beside candidates
def test_trajectory_against_the_twin(name, sw, options):
    ref = twin("%s/%d" % (name, sw))
    assert ref["accepted"] >= 3 and ref["restarts"] >= 1                # the window exercises what it is meant to
    s = run(name, 60, sw, dict(options or {}, accel=5))
    ai = s.accel_info()
    head = ref["first_accept"]                                          # iterations 1 .. head: nothing amplified yet
    dev = {}
    for nm in ("errRp", "errRd", "pobj", "dobj", "relgap"):
        got, want = s.info_arr(nm), np.array(ref[nm])
        assert got.size == want.size == 60
        dev[nm] = rel_dev(got[:head], want[:head], nm), rel_dev(got[head:], want[head:], nm)
    tail_tol = max(d[0] for d in dev.values()) + 10 * ref["spread"]
    for nm, (dh, dt) in dev.items():
        print("%s sw=%d %s %s: head %.3e, tail %.3e (tolerance %.3e)" % (name, sw, options, nm, dh, dt, tail_tol))
        assert dh <= 1e-8, (nm, dh)
        assert dt <= tail_tol, (nm, dt, tail_tol)
    assert np.array_equal(s.info_arr("sig"), np.array(ref["sig"]))
    # the same decisions in the same order
    assert (ai["taken"], ai["accepted"], ai["rejected"], ai["restarts"]) == (ref["taken"], ref["accepted"], ref["rejected"], ref["restarts"])


# ------------------------------------------------------------------------------------------------------------- safeguard drill
@pytest.mark.parametrize("options", [None, {"host_solve": 1}], ids=["default", "host_solve"])
@pytest.mark.parametrize("sw", [ADMM, SGS], ids=["ADMM", "sGS"])
@pytest.mark.parametrize("name", ["pendulum_N=80", "closed"])
def test_safeguard_drill(name, sw, options):
    """accel_safeguard = 0 rejects every candidate: the run is the plain run plus one wasted iteration per rejection.  40 iterations:
    below the second sigma update (iteration 51), which counts engine iterations.  host_solve: y, Rp and the fetched vectors are
    restored on the host."""
    N = 40
    s = run(name, N, sw, dict(options or {}, accel=5, accel_safeguard=0))
    ai = s.accel_info()
    assert ai["accepted"] == 0 and ai["rejected"] == ai["taken"] > 0
    plain = run(name, N - ai["rejected"], sw, options)
    assert np.array_equal(s.X, plain.X) and np.array_equal(s.y, plain.y) and np.array_equal(s.S, plain.S)
    assert s.info_iter_num == N


@pytest.mark.parametrize("name", ["pendulum_N=80", "closed"])
def test_safeguard_drill_across_the_switch(name):
    """sGS until engine iteration 10, then ADMM with the best-iterate bookkeeping, every candidate rejected: the result -- the best
    iterate, restored at the end -- is the plain run's.  The switch counts engine iterations, so the plain run switches r1 iterations
    earlier, r1 = the rejections up to the switch; no snapshot may be taken of an iteration that started from a candidate.  (The
    restart AT the switch is counted in test_trajectory_against_the_twin[...-10]; here a rejection may empty the memory first.)"""
    N, opts = 40, {"accel": 5, "accel_safeguard": 0}
    r1 = run(name, CROSS, CROSS, opts).accel_info()["rejected"]
    s = run(name, N, CROSS, opts)
    ai = s.accel_info()
    assert r1 > 0 and ai["accepted"] == 0 and ai["rejected"] == ai["taken"] > r1
    plain = run(name, N - ai["rejected"], CROSS - r1)
    assert plain.state()["best_KKT"] > 0 and s.state()["best_KKT"] == plain.state()["best_KKT"]
    assert np.array_equal(s.X, plain.X) and np.array_equal(s.y, plain.y) and np.array_equal(s.S, plain.S)


def test_two_runs_agree_bit_for_bit():
    a, b = run("pendulum_N=80", 40, ADMM, {"accel": 8}), run("pendulum_N=80", 40, ADMM, {"accel": 8})
    assert a.accel_info()["accepted"] > 0
    for nm, va, vb in zip(list(INFO) + ["state", "info_iter_num", "X", "y", "S"], snapshot(a), snapshot(b)):
        assert np.array_equal(va, vb), nm


# ------------------------------------------------------------------------------------------------------------------ interplay
@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_update_bC_clears_the_memory(name):
    a = amd_problem(name)
    b = thin(a.b_indices, a.b_vals) if name == "closed" else (a.b_indices, a.b_vals)
    Cc = (a.C_indices, a.C_vals)
    b2, C2 = perturb(b[0], b[1], a.con_num), perturb(Cc[0], Cc[1], a.vec_len)
    u = solver({"accel": 5})
    init_with(u, a, b, Cc)
    u.solve(12, 0.0, 0, 50, 100, ADMM, 1.05)
    assert u.accel_info()["taken"] > 0
    X0, y0, S0, sig = u.X, u.y, u.S, u.state()["sig"]
    u.update_bC(b2[0], b2[1], C2[0], C2[1], True, sig)
    f = solver({"accel": 5})
    init_with(f, a, b2, C2, X0, y0, S0, sig)
    u.solve(15, 0.0, 0, 50, 100, ADMM, 1.05); f.solve(15, 0.0, 0, 50, 100, ADMM, 1.05)
    for nm, va, vb in zip(list(INFO) + ["state", "info_iter_num", "X", "y", "S"], snapshot(u), snapshot(f)):
        assert va.shape == vb.shape and np.array_equal(va, vb), nm


def test_a_continued_solve_starts_with_an_empty_memory():
    s = run("hinf12", 12, ADMM, {"accel": 5})
    assert s.accel_info()["columns"] > 0
    s.solve(0, 0.0, 0, 50, 100, ADMM, 1.05, if_first=False)
    assert s.accel_info()["columns"] == 0


def test_refusals():
    a = amd_problem("ublock")
    for kw in ({"world": 2}, {"eig_rank": 3}):
        s = solver({"accel": 5}, **kw)
        with pytest.raises(cuadmm_amd.CuadmmError) as e:
            s.init_problem(a)
        assert e.value.code == -1 and "accel" in str(e.value)
    q = make_synthetic([12] * 10 + [30] * 6, cons_per_block=4, seed=6, dense_C=False)
    s = solver({"accel": 5, "duo_share_device": 1})
    with pytest.raises(cuadmm_amd.CuadmmError) as e:
        s.duo_init(True, 2, 15, 30, q.vec_len, q.con_num, q.At_col_ptrs, q.At_row_ids, q.At_vals, len(q.At_vals), q.b_idx, q.b_vals, len(q.b_idx),
                   q.C_idx, q.C_vals, len(q.C_idx), q.blk, len(q.blk))
    assert e.value.code == -1 and "accel" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- convergence
# Inputs and parameters: where the numpy twin itself stays well inside the bounds below (NOTEBOOK.md, Round 7).  hinf12 does not reach
# 1e-3 within 20 000 iterations with or without acceleration, in either phase.  taha1a: with the sGS phase the twin's final objectives
# differ from the plain run's by 3.6e-3 relative, in the ADMM phase by 1.96e-3 -- 2 % under the bound of 2 x 1e-3, less room than a
# stopping iteration shifted by one takes (two runs that both stop at relgap < 1e-3 are not bound to agree better).  cnhil10 has
# pobj = 0.  truss5 in the ADMM phase (switch_admm = 0): the twin needs 6 762 iterations against 11 647, objectives within 3.5e-4.
# (With the sGS phase truss5 needs about 20 000 plain iterations and runs that long; the plateau it stops on moves the stopping iteration
# by hundreds between the engine and numpy.)  MAX_ITER leaves the plain run more than three times the twin's count.
CONV_INPUTS = ["truss5"]
MAX_ITER = 40000


@pytest.mark.parametrize("name", CONV_INPUTS)
def test_accelerated_run_converges_to_the_same_objectives(name):
    """a guard, not a performance claim: to 1e-3, accel = 5, ADMM phase"""
    tol = 1e-3
    plain, acc = run(name, MAX_ITER, ADMM, None, tol), run(name, MAX_ITER, ADMM, {"accel": 5}, tol)
    n0, n1 = plain.info_iter_num, acc.info_iter_num
    sp, sa = plain.state(), acc.state()
    print("%s: plain %d iterations, accel = 5 %d; %s" % (name, n0, n1, acc.accel_info()))
    for k in ("pobj", "dobj"):
        print("%s %s: plain %.10g, accel %.10g, relative difference %.3e" % (name, k, sp[k], sa[k], abs(sa[k] - sp[k]) / abs(sp[k])))
    assert n0 < MAX_ITER and n1 < MAX_ITER
    assert max(sp["errRp"], sp["errRd"], sp["relgap"]) < tol and max(sa["errRp"], sa["errRd"], sa["relgap"]) < tol
    for k in ("pobj", "dobj"):
        assert abs(sa[k] - sp[k]) <= 2 * tol * abs(sp[k]), (k, sa[k], sp[k])
    assert n1 <= 2 * n0
