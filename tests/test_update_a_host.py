"""cuadmm_aat_refactor (numeric refactorisation on the analysis of an existing factor) without a device: against a fresh
cuadmm_aat_create / _create_split with the same new values, bit for bit; plus the declarations and wrappers of cuadmm_update_A."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import cuadmm_amd
from cuadmm_amd._lib import PROTOTYPES, check
from oracle import cuadmm_oracle as orc
from tests.conftest import ROOT, load_npz_problem

LIBDIR = os.path.join(ROOT, "cuadmm_amd", "lib")
lib = cuadmm_amd.load()


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def _A(name, problem_dirs):
    p = orc.load_problem_txt(problem_dirs[name]) if name in problem_dirs else load_npz_problem(name)
    At = sp.csc_matrix((p.At_vals, p.At_row_ids, p.At_col_ptrs), shape=(p.vec_len, p.con_num))
    A = At.T.tocsc(); A.sort_indices()
    return p.con_num, p.vec_len, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def _create(m, L, cp, ri, vx, max_k):
    h = C.c_void_p()
    if max_k == 0:
        check(lib.cuadmm_aat_create(m, L, P(cp), P(ri), P(vx), 1e-15, C.byref(h)))
    else:
        check(lib.cuadmm_aat_create_split(m, L, P(cp), P(ri), P(vx), 1e-15, max_k, C.byref(h)))
    return h


def _arrays(h, m, schur=True):
    """copies of everything the factor holds: perm, Lp, Li, Lx, D and the Schur complement triplets"""
    k = lib.cuadmm_aat_tail_k(h)
    Lp, Li, Lx, D = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(lib.cuadmm_aat_factor_arrays(h, C.byref(Lp), C.byref(Li), C.byref(Lx), C.byref(D)))
    Lp, Li = C.cast(Lp, C.POINTER(C.c_int64)), C.cast(Li, C.POINTER(C.c_int))
    Lx, D = C.cast(Lx, C.POINTER(C.c_double)), C.cast(D, C.POINTER(C.c_double))
    Lp = np.ctypeslib.as_array(Lp, shape=(m + 1,)).copy()
    nst = int(Lp[m - k])                                       # a split factor stores the leading columns only
    out = {"perm": np.ctypeslib.as_array(lib.cuadmm_aat_perm(h), shape=(m,)).copy(), "Lp": Lp,
           "Li": np.ctypeslib.as_array(Li, shape=(nst,)).copy() if nst else np.zeros(0, np.int32),
           "Lx": np.ctypeslib.as_array(Lx, shape=(nst,)).copy() if nst else np.zeros(0),
           "D": np.ctypeslib.as_array(D, shape=(m,)).copy(), "k": k}
    if k > 0 and schur:
        rp, ci, vv = C.POINTER(C.c_int64)(), C.POINTER(C.c_int)(), C.POINTER(C.c_double)()
        check(lib.cuadmm_aat_tail_schur(h, C.byref(rp), C.byref(ci), C.byref(vv)))
        rp = np.ctypeslib.as_array(rp, shape=(k + 1,)).copy()
        out["srp"] = rp
        out["sci"] = np.ctypeslib.as_array(ci, shape=(int(rp[-1]),)).copy()
        out["sv"] = np.ctypeslib.as_array(vv, shape=(int(rp[-1]),)).copy()
    return out


def _same(a, b, numeric_only=False):
    keys = ("Lx", "D", "sv") if numeric_only else a.keys()
    for key in keys:
        if key in a or key in b:
            assert np.array_equal(a[key], b[key]), key


# the last is run split: with the planner's tail and with a forced small tail (both above the 512 rows from which the tail rows
# run on the host pool, and truss5 / hinf12 forced below it: the serial loop)
CASES = [("hinf12", 0), ("hinf12", -5), ("truss5", 0), ("truss5", -100), ("pendulum_N=80", 0), ("pendulum_N=80", 32768), ("pendulum_N=80", -1024)]


@pytest.mark.parametrize("name,max_k", CASES)
def test_refactor_equals_a_fresh_create_bit_for_bit(name, max_k, problem_dirs):
    m, L, cp, ri, vx = _A(name, problem_dirs)
    new = vx * (1.0 + 0.05 * np.cos(np.arange(vx.size, dtype=np.float64)))
    h = _create(m, L, cp, ri, vx, max_k)
    assert lib.cuadmm_aat_pattern_nnz(h) == vx.size and lib.cuadmm_aat_valid(h) == 1
    first = _arrays(h, m)
    if max_k != 0:
        assert first["k"] > 0
        lib.cuadmm_aat_tail_schur_release(h)                     # as the engine does after init: recomputed by the refactorisation
    check(lib.cuadmm_aat_refactor(h, P(new)))
    got = _arrays(h, m)
    fresh_h = _create(m, L, cp, ri, new, max_k)
    fresh = _arrays(fresh_h, m)
    # the solves on the refactored factor while it holds the NEW values, against the fresh one (one-piece: the permuted solve; split:
    # both leading sweeps)
    rhs = np.random.default_rng(5).standard_normal(m)
    xa, xb = rhs.copy(), rhs.copy()
    if first["k"] == 0:
        check(lib.cuadmm_aat_solve_permuted(h, P(rhs), P(xa))); check(lib.cuadmm_aat_solve_permuted(fresh_h, P(rhs), P(xb)))
    else:
        for fn in (lib.cuadmm_aat_solve_leading_forward, lib.cuadmm_aat_solve_leading_backward):
            check(fn(h, first["k"], P(xa))); check(fn(fresh_h, first["k"], P(xb)))
    assert np.array_equal(xa, xb)
    lib.cuadmm_aat_free(fresh_h)
    for key in ("perm", "Lp", "Li", "k"):                          # the analysis is untouched
        assert np.array_equal(got[key], first[key]), key
    _same(got, fresh)
    assert not np.array_equal(got["Lx"], first["Lx"]) or got["Lx"].size == 0
    # back to the original values: the original factor, bit for bit
    check(lib.cuadmm_aat_refactor(h, P(vx)))
    _same(_arrays(h, m), first)
    # the solves run on the refactored factor (one-piece: the permuted solve; split: the leading sweeps)
    rhs = np.random.default_rng(5).standard_normal(m)
    ref_h = _create(m, L, cp, ri, vx, max_k)
    a, b = rhs.copy(), rhs.copy()
    if first["k"] == 0:
        check(lib.cuadmm_aat_solve_permuted(h, P(rhs), P(a))); check(lib.cuadmm_aat_solve_permuted(ref_h, P(rhs), P(b)))
    else:
        check(lib.cuadmm_aat_solve_leading_forward(h, first["k"], P(a))); check(lib.cuadmm_aat_solve_leading_forward(ref_h, first["k"], P(b)))
    assert np.array_equal(a, b)
    lib.cuadmm_aat_free(ref_h); lib.cuadmm_aat_free(h)


def test_non_finite_values_are_refused_with_the_factor_unchanged(problem_dirs):
    m, L, cp, ri, vx = _A("truss5", problem_dirs)
    for max_k in (0, -100):
        h = _create(m, L, cp, ri, vx, max_k)
        before = _arrays(h, m)
        for bad in (np.nan, np.inf, -np.inf):
            v = vx.copy(); v[v.size // 2] = bad
            assert lib.cuadmm_aat_refactor(h, P(v)) == -1           # CUADMM_ERR_INVALID
            assert b"finite" in lib.cuadmm_last_error()
            assert lib.cuadmm_aat_valid(h) == 1
            _same(_arrays(h, m), before)
        assert lib.cuadmm_aat_refactor(None, P(vx)) == -1
        assert lib.cuadmm_aat_refactor(h, None) == -1
        _same(_arrays(h, m), before)
        lib.cuadmm_aat_free(h)


def test_zero_pivot_fails_like_a_fresh_create_and_a_later_refactor_recovers():
    """A = [[1, 0], [0, 1]] -> all-zero values with eps = 0: A A^T = 0, the first pivot is zero.  cuadmm_aat_create fails on these
    values with CUADMM_ERR_FACTOR; so does the refactorisation, which leaves the factor marked unusable until good values arrive."""
    cp, ri = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    good, zero = np.array([1.0, 2.0]), np.zeros(2)
    h = C.c_void_p()
    assert lib.cuadmm_aat_create(2, 2, P(cp), P(ri), P(zero), 0.0, C.byref(h)) == -4        # CUADMM_ERR_FACTOR
    check(lib.cuadmm_aat_create(2, 2, P(cp), P(ri), P(good), 0.0, C.byref(h)))
    before = _arrays(h, 2)
    assert lib.cuadmm_aat_refactor(h, P(zero)) == -4
    assert lib.cuadmm_aat_valid(h) == 0
    check(lib.cuadmm_aat_refactor(h, P(good)))
    assert lib.cuadmm_aat_valid(h) == 1
    _same(_arrays(h, 2), before)
    lib.cuadmm_aat_free(h)


def test_symbols_are_exported_with_the_declared_signatures():
    hdr = open(os.path.join(ROOT, "include", "cuadmm_amd.h")).read()
    want = {"cuadmm_update_A": ["cuadmm_solver* s", "const double* At_csc_vals", "int At_nnz", "int keep_iterate", "double sig"],
            "cuadmm_get_update_info": ["const cuadmm_solver* s", "double out6[6]"],
            "cuadmm_aat_refactor": ["cuadmm_aat* f", "const double* A_vals"]}
    dll = C.CDLL(cuadmm_amd.LIB_PATH)
    for name, args in want.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name + " is not declared in include/cuadmm_amd.h"
        assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == args
        getattr(dll, name)
        assert name in PROTOTYPES
    assert PROTOTYPES["cuadmm_update_A"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double])


def test_uninitialised_handle_is_refused():
    h = C.c_void_p()
    assert lib.cuadmm_create(C.byref(h)) == 0
    try:
        v = (C.c_double * 2)(1.0, 2.0)
        assert lib.cuadmm_update_A(h, v, 2, 1, 0.0) == -1
        assert b"not initialised" in lib.cuadmm_last_error()
        o = (C.c_double * 6)()
        assert lib.cuadmm_get_update_info(h, o) == 0 and list(o) == [0.0] * 6
    finally:
        lib.cuadmm_destroy(h)
    assert lib.cuadmm_update_A(None, None, 0, 1, 0.0) == -1


def test_python_wrapper_has_the_methods():
    sig = inspect.signature(cuadmm_amd.SDPSolver.update_A)
    assert list(sig.parameters) == ["self", "vals", "keep_iterate", "sig"]
    assert sig.parameters["keep_iterate"].default is True and sig.parameters["sig"].default == 0.0
    s = cuadmm_amd.SDPSolver(verbose=False)
    assert list(s.update_info()) == [0.0] * 6
    with pytest.raises(cuadmm_amd.CuadmmError) as e:
        s.update_A([1.0])
    assert e.value.code == -1 and "not initialised" in str(e.value)


CALLER = r'''
#include <iostream>
#include <vector>

#include "cuadmm_amd.hpp"

int main() {
  try {
    cuadmm_amd::SDPSolver solver;
    std::vector<double> v{1.0, 2.0};
    solver.update_A(v.data(), 2);                 // warm start, sigma kept
    solver.update_A(v.data(), 2, false, 2.0);
  } catch (const std::exception& e) {
    std::cerr << "cuadmm_amd: " << e.what() << std::endl;
    return 3;
  }
  return 0;
}
'''


def test_cpp_facade_caller_compiles_and_links(tmp_path):
    src = tmp_path / "caller.cpp"
    src.write_text(CALLER)
    exe = tmp_path / "caller"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + LIBDIR, "-lcuadmm_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "not initialised" in r.stderr


def test_cli_refuses_an_unreadable_then_A_directory(tmp_path, problem_dirs):
    exe = os.path.join(LIBDIR, "cuadmm_exe")
    missing = str(tmp_path / "no_such_dir") + "/"
    r = subprocess.run([exe, problem_dirs["hinf12"], "--then-A=" + missing, "--quiet", "--max_iter=1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "cannot read --then-A directory" in r.stderr and "no_such_dir" in r.stderr
    assert not os.path.exists(os.path.join(problem_dirs["hinf12"], "X_opt.txt"))       # refused before any work
