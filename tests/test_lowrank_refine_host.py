"""cuadmm_lowrank_refine without a device: the host-only scalar step cuadmm_cg_update against the header's formula bit for bit, its
refusals, the declarations in the C header, the C++ facade and the ctypes table, the word cuadmm_op_check_factors learns, and the Python
front end's refusals (include/cuadmm_amd.h; csrc/cg_update.cpp; tests/_lowrank_refine_twin.py; cuadmm_amd/solver.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd import _lib
from cuadmm_amd.solver import lowrank_refine_args
from tests._lowrank_refine_twin import cg_update as twin_update

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def raw(gg, go, gd, gg_prev, first):
    o = np.full(3, np.nan)
    rc = cuadmm_amd.load().cuadmm_cg_update(float(gg), float(go), float(gd), float(gg_prev), int(first), P(o))
    return rc, o


def same(o, want):
    w = np.array([want[0], want[1], 1.0 if want[2] else 0.0])
    return np.array_equal(o.view(np.uint64), w.view(np.uint64))


def test_cg_update_is_the_formula_bit_for_bit():
    rng = np.random.default_rng(5)
    seen = {"pr+": 0, "restart": 0, "clamped": 0}
    for i in range(2000):
        gg, gp = (abs(rng.standard_normal()) * 10.0 ** rng.integers(-6, 7) for _ in range(2))
        go, gd = (rng.standard_normal() * 10.0 ** rng.integers(-6, 7) for _ in range(2))
        first = i % 17 == 0
        rc, o = raw(gg, go, gd, gp, first)
        want = twin_update(gg, go, gd, gp, first)
        assert rc == 0 and same(o, want), (gg, go, gd, gp, first, o, want)
        seen["pr+"] += o[0] > 0
        seen["restart"] += o[2] == 1 and not first
        seen["clamped"] += gg - go < 0 and not first
    assert min(seen.values()) > 100, seen


def test_cg_update_named_cases():
    # first: beta 0, restart, slope -gg whatever the other sums are
    assert same(raw(4.0, 1.0, 100.0, 2.0, 1)[1], (0.0, -4.0, True))
    # gg_prev = 0: beta 0, no division
    assert same(raw(4.0, 1.0, 100.0, 0.0, 0)[1], (0.0, -4.0, False))
    # a negative Polak-Ribiere numerator is clamped: steepest descent without the restart flag
    assert same(raw(1.0, 3.0, 5.0, 2.0, 0)[1], (0.0, -1.0, False))
    # beta = 1.5, slope = 1.5 * -1 - 2 < 0
    assert same(raw(2.0, 0.5, -1.0, 1.0, 0)[1], (1.5, -3.5, False))
    # slope >= 0 forces the restart with beta = 0; the slope returned is the one that forced it
    assert same(raw(2.0, 0.5, 3.0, 1.0, 0)[1], (0.0, 2.5, True))
    assert same(raw(3.0, 0.0, 1.0, 1.0, 0)[1], (0.0, 0.0, True))            # slope exactly 0
    # gg = 0: slope is -0.0 + 0 = 0, not negative: restart
    assert raw(0.0, 0.0, 0.0, 1.0, 0)[1][2] == 1.0
    # an overflowing quotient: beta = inf, slope = inf or NaN, never "negative": restart with beta = 0
    rc, o = raw(1e300, -1e300, 1.0, 1e-300, 0)
    assert rc == 0 and o[0] == 0.0 and o[2] == 1.0
    rc, o = raw(1e300, -1e300, 0.0, 1e-300, 0)                               # inf * 0 = NaN
    assert rc == 0 and o[0] == 0.0 and np.isnan(o[1]) and o[2] == 1.0
    assert twin_update(1e300, -1e300, 0.0, 1e-300, False)[2] is True


def test_cg_update_refuses_what_is_not_finite():
    lib = cuadmm_amd.load()
    good = [2.0, 0.5, -1.0, 1.0]
    for at in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            a = list(good)
            a[at] = bad
            rc, o = raw(*a, 0)
            assert rc == -1 and np.all(np.isnan(o)) and b"cg_update" in lib.cuadmm_last_error()
    assert lib.cuadmm_cg_update(2.0, 0.5, -1.0, 1.0, 0, None) == -1
    with pytest.raises(cuadmm_amd.CuadmmError):
        cuadmm_amd.cg_update(np.nan, 0.0, 0.0, 1.0, False)
    assert cuadmm_amd.cg_update(2.0, 0.5, -1.0, 1.0, False) == {"beta": 1.5, "slope": -3.5, "restart": False}


def _decl(header, name):
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, header, re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_facade_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "cuadmm_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "cuadmm_amd.hpp")).read()
    lib = cuadmm_amd.load()
    kinds = {"double": C.c_double, "int": C.c_int, "long long": C.c_longlong}
    for name in ("cuadmm_lowrank_refine", "cuadmm_cg_update", "cuadmm_op_lrr_dots", "cuadmm_op_lrr_direction", "cuadmm_op_lrr_step"):
        args = _decl(header, name)
        res, types = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == len(types), name
        for a, t in zip(args, types):
            if "*" in a or "[" in a:
                assert t is C.c_void_p, (name, a)
            else:
                assert t is kinds[a.rsplit(" ", 1)[0]], (name, a)
        assert getattr(lib, name).argtypes == types
    args = _decl(header, "cuadmm_lowrank_refine")
    assert [a.split()[-1].split("[")[0].lstrip("*") for a in args] == ["s", "L", "ranks", "rmax", "y", "sigma", "steps", "t_max", "gtol", "L_out", "trace", "out8", "r_out"]
    # the facade passes the thirteen arguments in the header's order
    m = re.search(r"check\(cuadmm_lowrank_refine\(([^;]*)\)\);", hpp)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["h_", "L", "ranks", "rmax", "y", "sigma", "steps", "t_max", "gtol", "g.L.data()", "g.trace.data()",
                                                                 "o", "g.r.data()"]
    assert "LowRankRefine lowrank_refine(const double* L, const int* ranks, int rmax, const double* y = nullptr, double sigma = 1.0, int steps = 10," in hpp
    # the binding's defaults are the issue's
    import inspect
    sig = inspect.signature(cuadmm_amd.SDPSolver.lowrank_refine)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[2:]] == [("y", None), ("sigma", 1.0), ("steps", 10), ("t_max", float("inf")), ("gtol", 0.0)]
    assert "cg_update" in cuadmm_amd.__all__


def test_check_factors_knows_the_word():
    lib = cuadmm_amd.load()
    b, r = np.array([3, -2, 4], np.int32), np.array([1, 0, 2], np.int32)
    L = np.zeros(3 * 2 + 4 * 2)                                              # block 0: min(3, rmax) columns of 3, block 2: 2 columns of 4
    assert lib.cuadmm_op_check_factors(b"lowrank_refine", P(b), 3, P(r), 2, P(L), None) == 0
    L[6 + 4 + 1] = np.nan                                                    # block 2, column 1, row 1
    assert lib.cuadmm_op_check_factors(b"lowrank_refine", P(b), 3, P(r), 2, P(L), None) == -1
    assert lib.cuadmm_last_error().decode() == "lowrank_refine: block 2, row 1 of column 1 is not finite"
    r[2] = 1                                                                 # the column is no longer read
    assert lib.cuadmm_op_check_factors(b"lowrank_refine", P(b), 3, P(r), 2, P(L), None) == 0
    r[0] = 3
    assert lib.cuadmm_op_check_factors(b"lowrank_refine", P(b), 3, P(r), 2, P(L), None) == -1
    assert lib.cuadmm_last_error().decode() == "lowrank_refine: block 0 of size 3 has rank 3, allowed are 0 to 2"


def test_the_front_end_refuses_before_the_library():
    blk, m = [3, -2, 4], 5
    Ls = [np.ones((3, 1)), np.zeros((0, 0)), np.ones((4, 2))]
    Lv, ranks, rmax, y, sigma, steps, t_max, gtol = lowrank_refine_args(blk, m, Ls, np.arange(5.0), 0.5, 3, 2.0, 1e-3)
    assert Lv.size == 3 * 2 + 4 * 2 and ranks.tolist() == [1, 0, 2] and rmax == 2 and (sigma, steps, t_max, gtol) == (0.5, 3, 2.0, 1e-3)
    for args in ((Ls, None, -1.0, 3, 1.0, 0.0), (Ls, None, np.nan, 3, 1.0, 0.0), (Ls, None, 1.0, 0, 1.0, 0.0), (Ls, None, 1.0, 3, 0.0, 0.0),
                 (Ls, None, 1.0, 3, np.nan, 0.0), (Ls, None, 1.0, 3, 1.0, -1.0), (Ls, None, 1.0, 3, 1.0, np.nan), (Ls, None, 1.0, 3, 1.0, np.inf),
                 (Ls[:2], None, 1.0, 3, 1.0, 0.0), (Ls, np.zeros(4), 1.0, 3, 1.0, 0.0)):
        with pytest.raises(ValueError, match="lowrank_refine"):
            lowrank_refine_args(blk, m, *args)
