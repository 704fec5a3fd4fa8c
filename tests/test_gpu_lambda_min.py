"""Certified lambda_min on the GPU (include/cuadmm_amd.h: cuadmm_lambda_min, cuadmm_op_block_lambda_min; DESIGN.md, "Certified
lambda_min"; csrc/lambda_min.hip; csrc/engine_reports.hip: lm_run): the kernel on every size class and matrix family of
tests/_lambda_min_twin.py against the two properties stated there, then the solver entry: its three matrices, LB_lambda against
cuadmm_lower_bound and a known optimum, the DIMACS measures against cuadmm_evaluate's Frobenius ones, no side effects, refusals, and the
three front ends.

Tolerances, none of them measured:
  validity, tightness   lam_ref = eigvalsh, e_ref = n 2^-52 ||M||_F (0 where lambda_min is known exactly); the margin is the library's
  which = 2             e_ref plus form_error (tests/_lower_bound_twin.py): numpy and the engine round C - A'y differently
  LB_lambda <= p*       sum_k R_k form_error_k + 64 2^-53 (|b'y| + |b|'|y|): the rounding of S^ and of b'y, which no bound on
                        lambda_min covers
  err2 / err4           [2] <= err + (margin and floor of the worst block) / (1 + norm), [2] >= err / sqrt(sum n_k) - the same
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd.devbuf import Dev
from tests._lambda_min_twin import (AT_FLOOR, FREE, REFINED, SIZE_CLASSES, UNREFINED, bracket, cases, check_properties, margin, reference,
                                    unpack)
from tests._lower_bound_twin import blk_lens, form_error, make_opt_fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
BLK_A, M_A = [3, 20, 70, -2, 130], 40          # the evaluation's fixture A (tests/test_gpu_evaluate.py): four size classes and a free block
INFO = ("pobj", "dobj", "errRp", "errRd", "relgap", "sig", "bscale", "Cscale")
_fx = {}


def fixture():
    if "A" not in _fx:
        _fx["A"] = make_opt_fixture(BLK_A, M_A, 1)
    return _fx["A"]


def amd(fx):
    r, c, v = fx.coo()
    bi, ci = np.nonzero(fx.b)[0], np.nonzero(fx.C)[0]
    return cuadmm_amd.Problem.from_coo(fx.blk, fx.m, r, c, v, bi, fx.b[bi], ci, fx.C[ci])


def solver(fx, **kw):
    s = cuadmm_amd.SDPSolver(verbose=False, **kw)
    s.init_problem(amd(fx))
    return s


def op(vec, blk, T):
    lib = cuadmm_amd.load()
    blk = np.asarray(blk, np.int32)
    d = Dev(np.asarray(vec, np.float64))
    out = np.full(3 * blk.size, np.nan)
    rc = lib.cuadmm_op_block_lambda_min(d.ptr, P(blk), blk.size, T, P(out), None)
    assert rc == 0, lib.cuadmm_last_error()
    return out.reshape(-1, 3)


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SIZE_CLASSES))
def test_kernel_meets_validity_and_tightness(name):
    cs = cases(name)
    free = np.array([0.3, -0.4, 1.2])
    half = len(cs) // 2
    blk = [c[0] for c in cs[:half]] + [-3] + [c[0] for c in cs[half:]]          # a 'u' block in the middle of the list
    vec = np.concatenate([c[3] for c in cs[:half]] + [free] + [c[3] for c in cs[half:]])
    r12, r6 = op(vec, blk, 12), op(vec, blk, 6)
    assert tuple(r12[half]) == (0.0, 0.0, FREE) and tuple(r6[half]) == (0.0, 0.0, FREE)
    r12, r6 = np.delete(r12, half, axis=0), np.delete(r6, half, axis=0)
    count = {REFINED: 0, AT_FLOOR: 0, UNREFINED: 0}
    for (n, fam, M, v, exact), g12, g6 in zip(cs, r12, r6):
        lam, e = reference(M) if exact is None else (exact, 0.0)
        for T, g in ((12, g12), (6, g6)):
            check_properties(M, T, g[0], g[1], int(g[2]), lam, e, what=(n, fam, T))
        count[int(g12[2])] += 1
        t, f, nu_floor, nu_max = bracket(M)
        assert g6[0] <= g12[0] + margin(n, max(t, 0.0), abs(g12[0])), (n, fam)      # T = 6 and T = 12 bracket monotonically
        if fam == "tiny":
            assert g12[2] == UNREFINED and abs(g12[0] + nu_max) <= 1e-12 * nu_max
        if fam in ("neg_def", "indef_1e-3", "indef_1e-9"):
            assert g12[2] == REFINED and g12[0] < 0
        if fam == "zero":
            assert g12[0] == 0.0
    print(name, "flags of T = 12:", count)
    assert count[UNREFINED] == len(SIZE_CLASSES[name])
    assert np.array_equal(op(vec, blk, 12), np.insert(r12, half, [0.0, 0.0, FREE], axis=0))      # the same bits from run to run


def test_a_block_beyond_1024_is_flagged_without_a_trial():
    n = 1025
    rng = np.random.default_rng(5)
    d = 1.0 + rng.random(n)
    d[77] = -0.25
    M = np.diag(d)
    M[3, 900] = M[900, 3] = 0.5
    ii, jj = np.tril_indices(n)
    vec = M[ii, jj] * np.where(ii == jj, 1.0, np.sqrt(2.0))
    (lo, hi, flag), = op(vec, [n], 12)
    Mu = unpack(vec, n)
    lam, e = reference(Mu)
    t, f, nu_floor, nu_max = bracket(Mu)
    assert flag == UNREFINED and hi == -0.25
    assert lo <= lam + e and abs(lo + nu_max) <= 1e-12 * nu_max
    lib = cuadmm_amd.load()
    out = np.zeros(3)
    for T in (0, 41):
        assert lib.cuadmm_op_block_lambda_min(Dev(vec).ptr, P(np.array([n], np.int32)), 1, T, P(out), None) == -1


# ---- 2. the solver entry --------------------------------------------------------------------------------------------------
def _blocks(fx, v):
    off = np.concatenate([[0], np.cumsum(blk_lens(fx.blk))])
    return [None if n < 0 else unpack(v[off[k]:off[k + 1]], int(n)) for k, n in enumerate(fx.blk)]


def _hold(fx, got, v, what, extra=None):
    for k, M in enumerate(_blocks(fx, v)):
        if M is None:
            assert (got["lo"][k], got["hi"][k], got["flag"][k]) == (0.0, 0.0, FREE)
            continue
        lam, e = reference(M)
        check_properties(M, 12, got["lo"][k], got["hi"][k], int(got["flag"][k]), lam, e + (0.0 if extra is None else extra[k]), what=(what, k))
    psd = np.asarray(fx.blk) > 0
    assert got["lambda_min"] == got["lo"][psd].min() and got["block"] == int(np.flatnonzero(psd)[np.argmin(got["lo"][psd])])
    assert got["unrefined"] == int(np.sum(got["flag"] == UNREFINED)) and got["psd_at_floor"] == int(np.sum(got["flag"] == AT_FLOOR))
    assert got["ms"] > 0 and got["bytes"] > 0


@pytest.fixture(scope="module")
def solved():
    """fixture A after 150 iterations with trace bounds set: the three reports in the scaled state, then the bound, the evaluation and
    the iterate (which ends the scaled state), then the three reports again in the caller's units"""
    fx = fixture()
    s = solver(fx)
    s.set_trace_bounds(fx.R)
    s.solve(150, 1e-12)
    first = {w: s.lambda_min(w) for w in ("X", "S", "dual")}
    lb = s.lower_bound()
    ev = s.evaluate()
    X, y, S = s.X, s.y, s.S
    again = {w: s.lambda_min(w) for w in ("X", "S", "dual")}
    return fx, s, first, again, lb, ev, (X, y, S)


def test_the_three_matrices(solved):
    fx, s, first, again, lb, ev, (X, y, S) = solved
    Sh = fx.C - fx.A.T @ y
    fe = form_error(fx, y)
    for what, got in (("scaled state", first), ("caller's units", again)):
        _hold(fx, got["X"], X, what + " X")
        _hold(fx, got["S"], S, what + " S")
        _hold(fx, got["dual"], Sh, what + " dual", extra=fe)
        assert np.isnan(got["X"]["lower_bound"]) and np.isnan(got["S"]["lower_bound"])
        print(what, {w: (got[w]["lambda_min"], got[w]["block"], got[w]["dimacs"], got[w]["ms"]) for w in got})
    # the same kernel on the vectors the getters return
    for w, v in (("X", X), ("S", S)):
        r = op(v, fx.blk, 12)
        for k, M in enumerate(_blocks(fx, v)):
            if M is not None:
                lam, e = reference(M)
                check_properties(M, 12, r[k, 0], r[k, 1], int(r[k, 2]), lam, e, what=("op", w, k))
        assert np.array_equal(r[:, 2], again[w]["flag"]) and np.array_equal(r[:, 0], again[w]["lo"])      # caller's units: unit = 1, the same vector


def test_lower_bound_from_lambda_min(solved):
    fx, s, first, again, lb, ev, (X, y, S) = solved
    fe = form_error(fx, y)
    tol = float(np.sum(fx.R * fe)) + 64 * 2.0 ** -53 * (abs(fx.b @ y) + float(np.abs(fx.b) @ np.abs(y)))
    for what, got in (("scaled state", first["dual"]), ("caller's units", again["dual"])):
        LBl, LB = got["lower_bound"], lb["lower_bound"]
        print("%s: LB_lambda %.15g, LB %.15g, p* %.15g (tolerance %.3g)" % (what, LBl, LB, fx.pstar, tol))
        assert LBl >= LB - 1e-12 * (1 + abs(LB))
        assert LBl <= fx.pstar + tol
        psd = np.asarray(fx.blk) > 0
        pen = float(np.sum(fx.R[psd] * np.maximum(0.0, -got["lo"][psd])))
        off = np.concatenate([[0], np.cumsum(blk_lens(fx.blk))])
        Sh = fx.C - fx.A.T @ y
        pen += float(sum(fx.R[k] * np.linalg.norm(Sh[off[k]:off[k + 1]]) for k in np.flatnonzero(~psd)))
        assert abs(LBl - (float(fx.b @ y) - pen)) <= tol + 64 * 2.0 ** -53 * pen
    q = solver(fx)
    assert np.isnan(q.lambda_min("dual")["lower_bound"])                # no trace bounds: NaN


def test_dimacs_measures_against_the_frobenius_ones(solved):
    fx, s, first, again, lb, ev, (X, y, S) = solved
    psd = np.asarray(fx.blk) > 0
    root = np.sqrt(float(np.sum(np.asarray(fx.blk)[psd])))
    pb = ev["per_block"]
    for w, v, col, norm in (("X", X, 1, ev["norm_b"]), ("S", S, 3, ev["norm_C"])):
        got = first[w]
        fro = float(np.linalg.norm(pb[psd, col])) / (1 + norm)             # err2 / err4 over the PSD blocks
        k = got["block"]
        M = _blocks(fx, v)[k]
        t, f, nu_floor, nu_max = bracket(M)
        slack = (nu_floor + margin(M.shape[0], t, nu_floor) + 2e-12 * np.sqrt(blk_lens(fx.blk)[k]) * f) * 1.01 / (1 + norm)
        print("%s: DIMACS %.3e, Frobenius %.3e, slack %.3e" % (w, got["dimacs"], fro, slack))
        assert got["dimacs"] == max(0.0, -got["lambda_min"]) / (1 + norm)
        assert got["dimacs"] <= fro * 1.01 + slack
        assert got["dimacs"] >= fro / root - slack * len(fx.blk)
    assert ev["err2"] >= first["X"]["dimacs"] - 1e-12 and abs(ev["err2"] - float(np.linalg.norm(pb[psd, 1])) / (1 + ev["norm_b"])) <= 1e-15


def _traj(s):
    return [s.info_arr(k).copy() for k in INFO] + [s.X, s.y, s.S]


@pytest.mark.parametrize("mode", ["sgs", "admm"])
def test_the_call_leaves_the_iteration_alone(mode):
    fx = fixture()
    sw = 0 if mode == "admm" else int(1.1e4)
    runs = []
    for call in (True, False):
        s = solver(fx)
        s.set_trace_bounds(fx.R)
        s.solve(60, 0.0, switch_admm=sw)
        if call:
            for w in ("X", "S", "dual"):
                assert np.isfinite(s.lambda_min(w, steps=5)["lambda_min"])
        s.solve(60, 0.0, switch_admm=sw, if_first=False)
        runs.append(_traj(s))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_refusals():
    fx = fixture()
    lib = cuadmm_amd.load()
    o = np.zeros(8)
    s = solver(fx)
    for steps in (0, 41, -3):
        with pytest.raises(cuadmm_amd.CuadmmError, match="steps") as e:
            s.lambda_min("X", steps=steps)
        assert e.value.code == -1
    assert lib.cuadmm_lambda_min(s._h, 0, 12, None, None) == -1
    assert lib.cuadmm_lambda_min(s._h, 3, 12, P(o), None) == -1
    assert lib.cuadmm_lambda_min(None, 0, 12, P(o), None) == -1
    fresh = cuadmm_amd.SDPSolver(verbose=False)
    assert lib.cuadmm_lambda_min(fresh._h, 0, 12, P(o), None) == -1     # not initialised
    with pytest.raises(ValueError):
        s.lambda_min("y")
    w = cuadmm_amd.SDPSolver(verbose=False, rank=0, world=2)
    w.set_allreduce(lambda ptr, count, stream: None)
    w.init_problem(amd(fx))
    with pytest.raises(cuadmm_amd.CuadmmError, match="works on one rank") as e:
        w.lambda_min("X")
    assert e.value.code == -1
    # behind a failed cuadmm_update_A: X and S are still reported, the dual matrix is refused
    s.set_option("update_A_inject_fail", 1)                              # the test hook of tests/test_gpu_update_a.py
    with pytest.raises(cuadmm_amd.CuadmmError) as e:
        s.update_A(amd(fx).At_csc_vals * 1.5)
    assert e.value.code == -4
    assert np.isfinite(s.lambda_min("X")["lambda_min"])
    with pytest.raises(cuadmm_amd.CuadmmError, match="cuadmm_update_A") as e:
        s.lambda_min("dual")
    assert e.value.code == -4 == lib.cuadmm_evaluate(s._h, None, None, None, P(np.zeros(16)), None)     # CUADMM_ERR_FACTOR, as cuadmm_evaluate


# ---- 3. the three front ends ----------------------------------------------------------------------------------------------
FACADE = r'''
#include <cstdio>
#include <string>
#include <tuple>
#include <vector>

#include "cuadmm_amd.hpp"
using namespace cuadmm_amd;

int main(int argc, char* argv[]) {
  if (argc < 2) return 2;
  try {
    Problem problem;
    problem.from_txt(argv[1]);
    std::vector<int> blk_vals;
    for (const auto& b : problem.blk_vals) blk_vals.push_back(std::get<0>(b) == 'u' ? -std::get<1>(b) : std::get<1>(b));
    SDPSolver solver;
    solver.set_option("verbose", 0.0);
    solver.init(15, 30, problem.vec_len, problem.con_num, problem.At_csc_col_ptrs.data(), problem.At_csc_row_ids.data(), problem.At_csc_vals.data(),
                problem.At_nnz, problem.b_indices.data(), problem.b_vals.data(), problem.b_nnz, problem.C_indices.data(), problem.C_vals.data(),
                problem.C_nnz, blk_vals.data(), problem.mat_num, problem.X_vals.data(), problem.y_vals.data(), problem.S_vals.data(), 1.0);
    solver.solve(150, 1e-12, false, 50, 100, 5000);
    for (int w = 0; w < 3; ++w) {
      std::vector<double> pb;
      const SDPSolver::LambdaMin r = solver.lambda_min(w, 12, &pb);
      std::printf("LM %d %.17g %d %zu\n", w, r.lambda_min, r.block, pb.size());
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cuadmm_amd: %s\n", e.what());
    return 3;
  }
  return 0;
}
'''


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


def test_python_facade_and_command_line_agree(tmp_path):
    fx = fixture()
    d = str(tmp_path / "prob") + "/"
    _write_txt(d, fx)
    libdir = os.path.join(ROOT, "cuadmm_amd", "lib")
    prob = cuadmm_amd.Problem.from_txt(d)
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(prob)
    s.solve(150, 1e-12, 0, 50, 100, 5000, 1.05)
    want = [s.lambda_min(w) for w in ("X", "S", "dual")]
    # the command line
    js = str(tmp_path / "lm.json")
    r = subprocess.run([os.path.join(libdir, "cuadmm_exe"), d, "--lambda-min", "--max_iter=150", "--stop_tol=1e-12", "--quiet", "--json=" + js],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("lambda_min(") == 3 and "lambda_min(dual) >=" in r.stdout
    with open(js) as f:
        side = json.load(f)["lambda_min"]
    assert side["steps"] == 12
    # the C++ facade
    src, exe = tmp_path / "facade.cpp", tmp_path / "facade"
    src.write_text(FACADE)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + libdir,
                           "-lcuadmm_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([str(exe), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("LM ")]
    assert len(lines) == 3
    for w, name in enumerate(("X", "S", "dual")):
        a, b, c = want[w]["lambda_min"], side[name]["lambda_min"], float(lines[w][2])
        print(name, a, b, c)
        assert abs(a - b) <= 1e-15 * abs(a) and abs(a - c) <= 1e-15 * abs(a)
        assert side[name]["block"] == want[w]["block"] == int(lines[w][3]) and int(lines[w][4]) == 3 * len(fx.blk)
        assert side[name]["lower_bound"] is None                            # no trace bounds on this command line
    r = subprocess.run([os.path.join(libdir, "cuadmm_exe"), d, "--lambda-min=41", "--quiet"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "1 to 40" in r.stderr
