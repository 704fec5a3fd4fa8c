"""Per-block pivoted Cholesky on the GPU (include/cuadmm_amd.h: cuadmm_lowrank, cuadmm_lowrank_size, cuadmm_op_block_lowrank; DESIGN.md,
"Low-rank factors"; csrc/lowrank.hip; csrc/engine_reports.hip: lr_run): the kernel on every size class and matrix family of
tests/_lowrank_twin.py against the four statements checked there, then the solver entry: the kernel's bits on a fresh solver, the
statements behind a solve in the scaled state, no side effects, refusals, null outputs, the bytes held, and the three front ends.

Tolerances, none of them measured: those of tests/_lowrank_twin.py (check_properties), which tests/test_lowrank_host.py shows the numpy
twin alone to meet; behind a solve a further 8 u relative for the conversion of the scaled numbers to the caller's units (one rounding
each in bscale X, sqrt(bscale), sqrt(bscale) L and its square, the scaled threshold and sums)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd.devbuf import Dev
from tests._lower_bound_twin import blk_lens, make_opt_fixture
from tests._lowrank_twin import (CAPPED, COMPLETE, FREE, LAUNCHES, NOT_FACTORED, SIZES, TOL, U, cases, check_properties, lowrank_size, split, unpack)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
BLK_A, M_A = [3, 20, 70, -2, 130], 40          # the evaluation's fixture A (tests/test_gpu_evaluate.py): three size classes and a free block
K_MAX = 8192                                     # kMaxBlockSize (csrc/device_util.h)
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


def solver(fx, X=None, y=None, S=None, **kw):
    s = cuadmm_amd.SDPSolver(verbose=False, **kw)
    s.init_problem(amd(fx), X, y, S)
    return s


def op(vec, blk, tol, rmax, factors=True):
    """(per_block (mat_num, 6), L, piv) of cuadmm_op_block_lowrank"""
    lib = cuadmm_amd.load()
    blk = np.asarray(blk, np.int32)
    d = Dev(np.asarray(vec, np.float64))
    count = max(lowrank_size(blk, rmax), 1)
    pb = np.full(6 * blk.size, np.nan)
    L, piv = (np.full(count, np.nan), np.full(count, -7, np.int32)) if factors else (None, None)
    rc = lib.cuadmm_op_block_lowrank(d.ptr, P(blk), blk.size, tol, rmax, P(pb), P(L), P(piv), None)
    assert rc == 0, lib.cuadmm_last_error()
    return pb.reshape(-1, 6), L, piv


def raw(s, which, tol, rmax, factors=True, per_block=True):
    """(rc, out8, per_block (mat_num, 6), L, piv) of cuadmm_lowrank"""
    lib = cuadmm_amd.load()
    count = max(lowrank_size(s.blk_vals, rmax), 1)
    o = np.full(8, np.nan)
    pb = np.full(6 * s.mat_num, np.nan) if per_block else None
    L, piv = (np.full(count, np.nan), np.full(count, -7, np.int32)) if factors else (None, None)
    rc = lib.cuadmm_lowrank(s._h, which, tol, rmax, P(o), P(pb), P(L), P(piv))
    return rc, o, None if pb is None else pb.reshape(-1, 6), L, piv


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------
def _launch(name):
    cs = [c for n in LAUNCHES[name] for c in cases(n)]
    rmax = max(SIZES[n][0] for n in LAUNCHES[name])
    half = len(cs) // 2
    blk = [c["n"] for c in cs[:half]] + [-3] + [c["n"] for c in cs[half:]]          # a 'u' block in the middle of the list
    vec = np.concatenate([c["vec"] for c in cs[:half]] + [np.array([0.3, -0.4, 1.2])] + [c["vec"] for c in cs[half:]])
    return cs, rmax, half, blk, vec


@pytest.mark.parametrize("name", list(LAUNCHES))
def test_kernel_meets_the_four_statements(name):
    cs, rmax, half, blk, vec = _launch(name)
    pb, L, piv = op(vec, blk, TOL, rmax)
    assert L.size == lowrank_size(blk, rmax) and not np.any(np.isnan(L)) and not np.any(piv == -7)      # every entry is written
    parts = split(blk, rmax, pb, L, piv)
    assert tuple(pb[half, :5]) == (0.0, 0.0, 0.0, 0.0, FREE) and pb[half, 5] == pb[half + 1, 5]
    del parts[half]
    base = {}
    for c, (rank, resid, dneg, t, flag, Lk, pk) in zip(cs, parts):
        n, fam, M = c["n"], c["family"], c["M"]
        what = (name, n, fam)
        print(what, "rank", rank, "resid %.3e dneg %.3e flag %d" % (resid, dneg, flag))
        if fam == "nan":
            assert (rank, flag, dneg) == (0, NOT_FACTORED, 0.0) and np.isnan(resid) and np.all(Lk == 0.0) and np.all(pk == -1), what
            continue
        check_properties(M, TOL, rmax, rank, resid, dneg, flag, Lk, pk, psd=c["psd"], what=what)
        assert abs(t - np.trace(M)) <= n * U * np.abs(np.diag(M)).sum(), what
        if c["r0"] is not None:
            assert rank == min(c["r0"], rmax) and flag == (CAPPED if c["r0"] > rmax else COMPLETE), (what, rank, flag)
        if fam == "identity":
            assert np.array_equal(pk, np.arange(n)[:min(n, rmax)]), what               # ties: the smallest index
        if fam == "zero":
            assert (rank, resid, dneg, flag) == (0, 0.0, 0.0, COMPLETE), what
        if fam == "indef":
            assert dneg <= -0.25 and n // 2 not in pk[:rank].tolist(), (what, dneg)
        if fam == "lowrank_2":
            base[n] = (rank, flag, Lk, pk)
        if fam.startswith("scaled"):
            r0, f0, L0, p0 = base[n]
            assert (rank, flag) == (r0, f0) and np.array_equal(pk, p0) and np.array_equal(Lk, L0 * 2.0 ** (-200 if fam == "scaled_down" else 200)), what
    again = op(vec, blk, TOL, rmax)                                                    # the same bits from run to run
    assert np.array_equal(again[0], pb, equal_nan=True) and np.array_equal(again[1], L) and np.array_equal(again[2], piv)


def test_a_cap_of_one_column():
    cs = [c for n in (31, 65, 300) for c in cases(n) if c["family"] == "lowrank_5"]
    blk = [c["n"] for c in cs]
    pb, L, piv = op(np.concatenate([c["vec"] for c in cs]), blk, TOL, 1)
    for c, (rank, resid, dneg, t, flag, Lk, pk) in zip(cs, split(blk, 1, pb, L, piv)):
        assert (rank, flag) == (1, CAPPED) and pk[0] == int(np.argmax(np.diag(c["M"]))), (c["n"], rank, flag, pk)
        check_properties(c["M"], TOL, 1, rank, resid, dneg, flag, Lk, pk, what=(c["n"], "rmax = 1"))
    lib = cuadmm_amd.load()
    d, b, o = Dev(cs[0]["vec"]), np.array([31], np.int32), np.zeros(6)
    for tol, rmax in ((-1.0, 4), (1.0, 4), (float("nan"), 4), (1e-8, 0), (1e-8, K_MAX + 1)):
        assert lib.cuadmm_op_block_lowrank(d.ptr, P(b), 1, tol, rmax, P(o), None, None, None) == -1


# ---- 2. the solver entry --------------------------------------------------------------------------------------------------
def _blocks(fx, v):
    off = np.concatenate([[0], np.cumsum(blk_lens(fx.blk))])
    return [None if n < 0 else unpack(v[off[k]:off[k + 1]], int(n)) for k, n in enumerate(fx.blk)]


def _out8_is_consistent(o, pb):
    psd = pb[:, 4] != FREE
    assert o[0] == pb[psd, 0].sum() and o[1] == pb[psd, 0].max() and o[2] == np.flatnonzero(psd)[np.argmax(pb[psd, 0])]
    assert abs(o[3] - pb[psd, 1].sum()) <= len(pb) * U * pb[psd, 1].sum() and o[4] == min(0.0, pb[psd, 2].min())
    assert o[5] == np.sum(pb[:, 4] == CAPPED) and o[6] > 0 and o[7] > 0


def test_fresh_solver_runs_the_kernel_on_the_vectors_of_init():
    fx = fixture()
    s = solver(fx, fx.Xs, fx.ys, fx.Ss)
    rmax = max(BLK_A)
    count = C.c_longlong(0)
    lib = cuadmm_amd.load()
    for q in (1, 5, 70, rmax, K_MAX):
        assert lib.cuadmm_lowrank_size(s._h, q, C.byref(count)) == 0 and count.value == lowrank_size(fx.blk, q)
    # init holds X0 / bscale and S0 / Cscale, which the getters of a solver that has not solved return as they stand: those are the
    # vectors the report reads, as the other point reports do in this state
    for w, v in ((0, s.X), (1, s.S)):
        rc, o, pb, L, piv = raw(s, w, TOL, rmax)
        assert rc == 0, lib.cuadmm_last_error()
        want = op(v, fx.blk, TOL, rmax)
        assert np.array_equal(pb, want[0]) and np.array_equal(L, want[1]) and np.array_equal(piv, want[2])
        assert tuple(pb[3, :5]) == (0.0, 0.0, 0.0, 0.0, FREE)
        _out8_is_consistent(o, pb)
        for k, M in enumerate(_blocks(fx, v)):                                        # X* has rank max(1, n // 3), S* the rest
            if M is not None:
                n = fx.blk[k]
                assert pb[k, 0] == (max(1, n // 3) if w == 0 else n - max(1, n // 3)), (w, k, pb[k])


def test_behind_a_solve_the_scaled_iterate_is_reported_in_the_callers_units():
    fx = fixture()
    s = solver(fx)
    s.solve(3000, 1e-6)
    st = s.state()
    print("iterations", s.info_iter_num, "bscale", st["bscale"], "Cscale", st["Cscale"])
    rmax = max(BLK_A)
    got = [raw(s, w, TOL, rmax) for w in (0, 1)]                                      # scaled state: before any getter
    X, S = s.X, s.S
    ranks = []
    for (rc, o, pb, L, piv), v, name in zip(got, (X, S), "XS"):
        assert rc == 0
        _out8_is_consistent(o, pb)
        for k, (M, (rank, resid, dneg, t, flag, Lk, pk)) in enumerate(zip(_blocks(fx, v), split(fx.blk, rmax, pb, L, piv))):
            if M is None:
                assert (rank, flag) == (0, FREE)
                continue
            check_properties(M, TOL, rmax, rank, resid, dneg, flag, Lk, pk, psd=False, conv=8 * U, what=(name, k))
            assert abs(t - np.trace(M)) <= (M.shape[0] + 8) * U * np.abs(np.diag(M)).sum()
        ranks.append(pb[:, 0].astype(int))
    print("rank X_k + rank S_k:", (ranks[0] + ranks[1]).tolist(), "of n_k =", BLK_A)
    # caller's units from here on (the getters ended the scaled state): the kernel on the returned vectors, bit for bit
    for w, v in ((0, X), (1, S)):
        rc, o, pb, L, piv = raw(s, w, TOL, rmax)
        want = op(v, fx.blk, TOL, rmax)
        assert rc == 0 and np.array_equal(pb, want[0]) and np.array_equal(L, want[1]) and np.array_equal(piv, want[2])


def _traj(s):
    return [s.info_arr(k).copy() for k in INFO] + [s.X, s.y, s.S]


def test_the_call_leaves_the_iteration_alone():
    fx = fixture()
    runs = []
    for call in (True, False):
        s = solver(fx)
        s.solve(30, 0.0)
        if call:
            for w in (0, 1):
                assert raw(s, w, TOL, 16)[0] == 0
        s.solve(30, 0.0, if_first=False)
        runs.append(_traj(s))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_refusals_null_outputs_and_the_bytes_held():
    fx = fixture()
    lib = cuadmm_amd.load()
    s = solver(fx, fx.Xs, fx.ys, fx.Ss)
    o = np.zeros(8)
    for which, tol, rmax in ((0, -1.0, 8), (0, 1.0, 8), (0, float("nan"), 8), (0, 1e-8, 0), (0, 1e-8, K_MAX + 1), (2, 1e-8, 8)):
        assert lib.cuadmm_lowrank(s._h, which, tol, rmax, P(o), None, None, None) == -1, (which, tol, rmax)
    assert lib.cuadmm_lowrank(s._h, 0, 1e-8, 8, None, None, None, None) == -1           # out8 = NULL
    w = cuadmm_amd.SDPSolver(verbose=False, rank=0, world=2)
    w.set_allreduce(lambda ptr, count, stream: None)
    w.init_problem(amd(fx))
    with pytest.raises(cuadmm_amd.CuadmmError, match="works on one rank") as e:
        w.lowrank("X", tol=1e-8)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        s.lowrank("dual", tol=1e-8)
    with pytest.raises(TypeError):
        s.lowrank("X")                                                                  # tol has no default
    # the solver is usable behind every refusal; null outputs change nothing of the rest
    rc, o8, pb, L, piv = raw(s, 0, TOL, 8)
    assert rc == 0
    for factors, per_block in ((False, True), (True, False), (False, False)):
        rc2, o2, pb2, L2, piv2 = raw(s, 0, TOL, 8, factors=factors, per_block=per_block)
        assert rc2 == 0 and np.array_equal(o2[:6], o8[:6])
        assert pb2 is None or np.array_equal(pb2, pb)
        assert L2 is None or (np.array_equal(L2, L) and np.array_equal(piv2, piv))
    # bytes held: grow with rmax, stay when it shrinks
    b8 = o8[7]
    b64 = raw(s, 0, TOL, 64)[1][7]
    b4 = raw(s, 0, TOL, 4)[1][7]
    grow = 8 * (lowrank_size(fx.blk, 64) - lowrank_size(fx.blk, 8))
    assert b64 >= b8 + grow and b4 == b64, (b8, b64, b4)
    # behind a failed cuadmm_update_A the report still runs: it does not read A
    s.set_option("update_A_inject_fail", 1)                                             # the test hook of tests/test_gpu_update_a.py
    with pytest.raises(cuadmm_amd.CuadmmError) as e:
        s.update_A(amd(fx).At_csc_vals * 1.5)
    assert e.value.code == -4 and raw(s, 0, TOL, 8)[0] == 0


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
    solver.solve(200, 1e-3, false, 50, 100, 5000);
    for (int w = 0; w < 2; ++w) {
      const SDPSolver::LowRank r = solver.lowrank(w, 1e-8, 6);
      std::printf("LR %d %.0f %d %d %zu %zu", w, r.rank_sum, r.rank_max, r.block, r.per_block.size(), r.L.size());
      for (size_t k = 0; k < r.per_block.size() / 6; ++k) std::printf(" %.0f", r.per_block[6 * k]);
      std::printf("\n");
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cuadmm_amd: %s\n", e.what());
    return 3;
  }
  return 0;
}
'''


def test_python_facade_and_command_line_agree(tmp_path, problem_dirs):
    d = problem_dirs["hinf12"]                                                          # the smallest committed TXT input
    libdir = os.path.join(ROOT, "cuadmm_amd", "lib")
    prob = cuadmm_amd.Problem.from_txt(d)
    blk = [int(n) for n in prob.blk_vals]
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(prob)
    s.solve(200, 1e-3, 0, 50, 100, 5000, 1.05)
    want = {w: s.lowrank(w, tol=1e-8) for w in ("X", "S")}
    capped = {w: s.lowrank(w, tol=1e-8, rmax=6) for w in ("X", "S")}
    for w, got in want.items():
        for k, n in enumerate(blk):
            assert got["L"][k].shape == (max(n, 0), got["rank"][k]) and got["piv"][k].shape == (got["rank"][k],)
            assert np.all(got["L"][k][got["piv"][k], np.arange(got["rank"][k])] > 0)
        assert got["rank_sum"] == got["rank"].sum() and got["rank_max"] == got["rank"].max() and got["ms"] > 0
    # the command line: ranks in the sidecar, factors in files
    js, out = str(tmp_path / "lr.json"), str(tmp_path) + "/"
    r = subprocess.run([os.path.join(libdir, "cuadmm_exe"), d, "--lowrank=1e-8", "--lowrank-out=" + out, "--max_iter=200", "--quiet", "--json=" + js],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count(" rank(") == 2 and " rank(S): sum" in r.stdout
    with open(js) as f:
        side = json.load(f)["lowrank"]
    assert side["tol"] == 1e-8 and side["rmax"] == max(blk)
    for w in ("X", "S"):
        assert side[w]["rank"] == want[w]["rank"].tolist() and side[w]["flag"] == want[w]["flag"].tolist() and side[w]["rank_sum"] == want[w]["rank_sum"]
        for k, n in enumerate(blk):
            if n > 0:
                Lk = np.loadtxt(out + "L_%s_%d.txt" % (w, k), ndmin=1).reshape(want[w]["rank"][k], n).T
                # the dense writer prints 32 decimals: absolute 1e-32, the engine's L to the last bit of all but its tiniest entries
                assert np.allclose(Lk, want[w]["L"][k], rtol=4 * U, atol=1e-32), (w, k)
    # the C++ facade
    src, exe = tmp_path / "facade.cpp", tmp_path / "facade"
    src.write_text(FACADE)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + libdir,
                           "-lcuadmm_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([str(exe), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("LR ")]
    assert len(lines) == 2
    for w, name in enumerate(("X", "S")):
        got = capped[name]
        assert [int(x) for x in lines[w][7:]] == got["rank"].tolist() and int(lines[w][2]) == got["rank_sum"] and int(lines[w][3]) == got["rank_max"]
        assert int(lines[w][4]) == got["block"] and int(lines[w][5]) == 6 * len(blk) and int(lines[w][6]) == lowrank_size(blk, 6)
    for bad in ("--lowrank=1", "--lowrank=1e-8,0", "--lowrank=x"):
        r = subprocess.run([os.path.join(libdir, "cuadmm_exe"), d, bad, "--quiet"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "0 <= TOL < 1" in r.stderr, bad
