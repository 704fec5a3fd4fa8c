"""cuadmm_update_bC (new b / C on a factored solver) without a device: the symbol and its declared signature, the refusal of a
handle that was never initialised, the Python and C++ wrappers, and the command line's --then= argument."""
import ctypes as C
import inspect
import os
import re
import subprocess

import cuadmm_amd
from cuadmm_amd._lib import PROTOTYPES
from tests.conftest import ROOT

LIBDIR = os.path.join(ROOT, "cuadmm_amd", "lib")


def test_symbol_is_exported_with_the_declared_signature():
    hdr = open(os.path.join(ROOT, "include", "cuadmm_amd.h")).read()
    m = re.search(r"int\s+cuadmm_update_bC\s*\(([^)]*)\)\s*;", hdr)
    assert m, "cuadmm_update_bC is not declared in include/cuadmm_amd.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["cuadmm_solver* s", "const int* b_indices", "const double* b_vals", "int b_nnz", "const int* C_indices",
                    "const double* C_vals", "int C_nnz", "int keep_iterate", "double sig"]
    getattr(C.CDLL(cuadmm_amd.LIB_PATH), "cuadmm_update_bC")
    restype, argtypes = PROTOTYPES["cuadmm_update_bC"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double]


def test_uninitialised_handle_is_refused():
    lib = cuadmm_amd.load()
    h = C.c_void_p()
    assert lib.cuadmm_create(C.byref(h)) == 0
    try:
        assert lib.cuadmm_update_bC(h, None, None, -1, None, None, -1, 1, 0.0) == -1          # CUADMM_ERR_INVALID
        assert len(lib.cuadmm_last_error()) > 0
        idx, val = (C.c_int * 1)(0), (C.c_double * 1)(1.0)
        assert lib.cuadmm_update_bC(h, idx, val, 1, idx, val, 1, 0, 1.0) == -1
    finally:
        lib.cuadmm_destroy(h)
    assert lib.cuadmm_update_bC(None, None, None, -1, None, None, -1, 1, 0.0) == -1


def test_python_wrapper_has_the_method():
    sig = inspect.signature(cuadmm_amd.SDPSolver.update_bC)
    assert list(sig.parameters) == ["self", "b_idx", "b_val", "C_idx", "C_val", "keep_iterate", "sig"]
    assert sig.parameters["keep_iterate"].default is True and sig.parameters["sig"].default == 0.0
    s = cuadmm_amd.SDPSolver(verbose=False)
    try:
        s.update_bC([0], [1.0])
        raise AssertionError("an uninitialised solver accepted update_bC")
    except cuadmm_amd.CuadmmError as e:
        assert e.code == -1 and "not initialised" in str(e)


CALLER = r'''
#include <iostream>
#include <vector>

#include "cuadmm_amd.hpp"

int main() {
  try {
    cuadmm_amd::SDPSolver solver;
    std::vector<int> bi{0}, ci{0, 2};
    std::vector<double> bv{1.0}, cv{1.0, 1.0};
    solver.update_bC(bi.data(), bv.data(), 1, ci.data(), cv.data(), 2);                 // warm start, sigma kept
    solver.update_bC(nullptr, nullptr, -1, ci.data(), cv.data(), 2, false, 2.0);
  } catch (const std::exception& e) {
    std::cerr << "cuadmm_amd: " << e.what() << std::endl;
    return 3;
  }
  return 0;
}
'''


def test_cpp_facade_caller_compiles_and_links(tmp_path):
    cuadmm_amd.load()
    src = tmp_path / "caller.cpp"
    src.write_text(CALLER)
    exe = tmp_path / "caller"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + LIBDIR, "-lcuadmm_amd", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "not initialised" in r.stderr          # the handle was never initialised: refused, as an exception


def test_cli_refuses_an_unreadable_then_directory(tmp_path, problem_dirs):
    exe = os.path.join(LIBDIR, "cuadmm_exe")
    missing = str(tmp_path / "no_such_dir") + "/"
    r = subprocess.run([exe, problem_dirs["hinf12"], "--then=" + missing, "--quiet", "--max_iter=1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "--then" in r.stderr and "no_such_dir" in r.stderr
    assert not os.path.exists(os.path.join(problem_dirs["hinf12"], "X_opt.txt"))       # refused before any work
