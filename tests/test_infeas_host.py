"""Option "infeas_check" without a device: the numpy twin on the small problems, its certificates against the original data, the
decision rule of the library (cuadmm_infeas_decide) and the option's range (include/cuadmm_amd.h; csrc/infeas.hip;
tests/_infeas_twin.py).

Certificate bound.  verify_primal / verify_dual recompute the violation of the returned ray with numpy.linalg.eigvalsh on the
ORIGINAL data and multiply it by the reported radius: <= 1 + 1e-9.  The reported radius is scalar / (eta + eta_fl) with
eta_fl = 1e-12 sqrt(L) ||M||_F / ||d||: the violation is a cancellation result whose absolute error is a multiple of
eps ||M||_F, so scalar / eta alone would claim more than double precision can check (seen on P: 1 + 2.4e-7 with eta = 3e-11).
"""
import ctypes as C

import numpy as np
import pytest

import cuadmm_amd
from tests._infeas_twin import STATUS, decide, make_fixture, twin_solve, verify_dual, verify_primal

PERIOD, TOL, CAP = 50, 1e-6, 2000
_twins = {}


def twin(kind, sw, big=False):
    key = (kind, sw, big)
    if key not in _twins:
        _twins[key] = twin_solve(make_fixture(kind, big), PERIOD, TOL, CAP, 1e-6, switch_admm=sw)
    return _twins[key]


@pytest.mark.parametrize("sw", [11000, 0])
@pytest.mark.parametrize("kind,status", [("P", 3), ("D", 4)])
def test_twin_declares_within_the_cap(kind, status, sw):
    r = twin(kind, sw)
    print(kind, sw, STATUS[r.status], "at", r.iteration, "scalar %.6g eta %.3g radius %.3g" % (r.scalar, r.eta, r.radius))
    assert r.status == status and r.iteration <= CAP and r.iteration % PERIOD == 0 and r.iteration >= 2 * PERIOD
    assert r.scalar > 0 and r.eta <= TOL * r.scalar


@pytest.mark.parametrize("sw", [11000, 0])
def test_feasible_control_converges_without_a_verdict(sw):
    r = twin("F", sw)
    assert r.status == 1 and r.iteration < CAP
    assert all(decide(st, TOL)[0] == 0 for _, st in r.history)


@pytest.mark.parametrize("sw", [11000, 0])
def test_twin_certificates_against_the_original_data(sw):
    fp, fd = make_fixture("P"), make_fixture("D")
    rp, rd = twin("P", sw), twin("D", sw)
    e, v = verify_primal(fp, rp.y_cert, rp.radius)
    print("primal: b'y - 1 = %.2e, violation x radius = %.12f" % (e, v))
    assert abs(e) <= 1e-12 and v <= 1 + 1e-9
    e, v = verify_dual(fd, rd.X_cert, rd.radius)
    print("dual: <C, X> + 1 = %.2e, violation x radius = %.12f" % (e, v))
    assert abs(e) <= 1e-12 and v <= 1 + 1e-9


def _decide(lib, stats, tol):
    st = np.array(stats, np.float64)
    verdict, radius = C.c_int(-1), C.c_double(-1.0)
    rc = lib.cuadmm_infeas_decide(st.ctypes.data_as(C.c_void_p), tol, C.byref(verdict), C.byref(radius))
    assert rc == 0, lib.cuadmm_last_error()
    assert (verdict.value, radius.value) == decide(st, tol)[::3] or (np.isinf(radius.value) and np.isinf(decide(st, tol)[3]))
    return verdict.value, radius.value


def test_decide_through_the_library():
    """stats = [|dy|^2, b'dy, |dX|^2, C'dX, |P+(A'dy)|^2, |A dX|^2, |P+(-dX)|^2, -]"""
    lib = cuadmm_amd.load()
    nan = float("nan")
    tol = 1e-6
    # both verdicts (|dy| = 2, beta = 0.5, eta = 1e-7 / 2), and the radius scalar / eta
    v, r = _decide(lib, [4.0, 1.0, nan, nan, 1e-14, nan, nan, 0], tol)
    assert v == 3 and r == pytest.approx(0.5 / 0.5e-7, rel=1e-14)
    v, r = _decide(lib, [nan, nan, 4.0, -1.0, nan, 1e-14, 4e-16, 0], tol)
    assert v == 4 and r == pytest.approx(0.5 / 0.5e-7, rel=1e-14)
    # the larger of the two dual violations decides
    assert _decide(lib, [nan, nan, 4.0, -1.0, nan, 1e-16, 1e-10, 0], tol)[0] == 0
    assert _decide(lib, [nan, nan, 4.0, -1.0, nan, 1e-10, 1e-16, 0], tol)[0] == 0
    # the sign gates: b'dy <= 0, C'dX >= 0
    assert _decide(lib, [4.0, -1.0, nan, nan, 0.0, nan, nan, 0], tol)[0] == 0
    assert _decide(lib, [4.0, 0.0, nan, nan, 0.0, nan, nan, 0], tol)[0] == 0
    assert _decide(lib, [nan, nan, 4.0, 1.0, nan, 0.0, 0.0, 0], tol)[0] == 0
    assert _decide(lib, [nan, nan, 4.0, 0.0, nan, 0.0, 0.0, 0], tol)[0] == 0
    # eta = 0: a certificate with an infinite radius
    v, r = _decide(lib, [4.0, 1.0, nan, nan, 0.0, nan, nan, 0], tol)
    assert v == 3 and np.isinf(r)
    v, r = _decide(lib, [nan, nan, 4.0, -1.0, nan, 0.0, 0.0, 0], tol)
    assert v == 4 and np.isinf(r)
    # exactly at the threshold (|dy| = 1, beta = 0.5, eta = 2^-21 = tol beta with tol = 2^-20: all exact in binary), then a few ulps above
    t = 2.0 ** -20
    assert _decide(lib, [1.0, 0.5, nan, nan, (2.0 ** -21) ** 2, nan, nan, 0], t)[0] == 3
    assert _decide(lib, [1.0, 0.5, nan, nan, (2.0 ** -42) * (1 + 2.0 ** -48), nan, nan, 0], t)[0] == 0
    # NaN statistics: no verdict
    for k in (0, 1, 4):
        st = [4.0, 1.0, nan, nan, 1e-14, nan, nan, 0]
        st[k] = nan
        assert _decide(lib, st, tol)[0] == 0
    for k in (2, 3, 5, 6):
        st = [nan, nan, 4.0, -1.0, nan, 1e-14, 1e-14, 0]
        st[k] = nan
        assert _decide(lib, st, tol)[0] == 0
    assert _decide(lib, [4.0, 1.0, 4.0, -1.0, 1e-14, 1e-14, 1e-14, 0], nan)[0] == 0
    # with both sets of numbers the primal test is read first
    assert _decide(lib, [4.0, 1.0, 4.0, -1.0, 1e-14, 1e-14, 1e-14, 0], tol)[0] == 3
    assert lib.cuadmm_infeas_decide(None, tol, None, None) == -1


def test_option_range_and_status_before_a_solve():
    lib = cuadmm_amd.load()
    h = C.c_void_p()
    assert lib.cuadmm_create(C.byref(h)) == 0
    try:
        for bad in (1.0, -1.0, 2.5, 1e6 + 1, float("nan")):
            assert lib.cuadmm_set_option(h, b"infeas_check", bad) == -1 and b"infeas_check" in lib.cuadmm_last_error()
        for good in (2.0, 1e6, 50.0, 0.0):
            assert lib.cuadmm_set_option(h, b"infeas_check", good) == 0
        assert lib.cuadmm_set_option(h, b"infeas_tol", -1e-6) == -1 and lib.cuadmm_set_option(h, b"infeas_tol", float("nan")) == -1
        assert lib.cuadmm_set_option(h, b"infeas_tol", 1e-5) == 0 and lib.cuadmm_set_option(h, b"infeas_tol", 0.0) == 0
        o = np.ones(8)
        assert lib.cuadmm_get_status(h, o.ctypes.data_as(C.c_void_p)) == 0
        assert not o.any()
        y = np.zeros(4)
        assert lib.cuadmm_get_certificate(h, y.ctypes.data_as(C.c_void_p), None) == -1
    finally:
        lib.cuadmm_destroy(h)
