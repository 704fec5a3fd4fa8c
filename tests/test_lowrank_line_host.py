"""cuadmm_lowrank_line without a device: the host-only minimiser cuadmm_quartic_min against a brute-force check, its refusals, the task list
the outer-product launch walks, the longdouble twin against lowrank_grad's, and the Python front end's packing and refusals
(include/cuadmm_amd.h; csrc/quartic_min.cpp; tests/_lowrank_line_twin.py; cuadmm_amd/solver.py: lowrank_line_args, quartic_min)."""
import ctypes as C

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd.solver import lowrank_line_args
from tests._block_mult_twin import LD, lowrank_size
from tests._lower_bound_twin import make_opt_fixture
from tests._lowrank_grad_twin import twin as grad_twin
from tests._lowrank_line_twin import U, horner, horner_bar, twin

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
INF = float("inf")


def raw_min(c, t_max):
    c = np.ascontiguousarray(c, np.float64)
    o = np.full(4, np.nan)
    rc = cuadmm_amd.load().cuadmm_quartic_min(P(c), float(t_max), P(o))
    return rc, o


def brute_force(c, t_max, o):
    """The returned value is <= the Horner value at every point of a grid of 4001 points on [0, T] and at every real root of the derivative
    (numpy.roots) inside it; T = t_max, or Cauchy's bound on the derivative's roots for t_max = inf.  Slack: both sides are Horner values,
    each within 8 u sum |c_i| t^i of the quartic at its own t, so the sum of the two."""
    t, f, dec, ncrit = o
    assert 0 <= t <= t_max and f == horner(c, t) and dec == f - c[0] and ncrit in (0, 1, 2, 3)
    T = t_max
    if np.isinf(t_max):
        d = [c[1], 2 * c[2], 3 * c[3], 4 * c[4]]
        T = 1 + (max(abs(v) for v in d[:3]) / d[3] if c[4] > 0 else abs(d[0]) / d[1])
    pts = list(np.linspace(0.0, T, 4001))
    dc = np.array([4 * c[4], 3 * c[3], 2 * c[2], c[1]])
    if np.any(dc != 0):
        pts += [float(z.real) for z in np.roots(dc) if abs(z.imag) <= 1e-9 * max(1.0, abs(z)) and 0 <= z.real <= T]
    pts = np.array(pts)
    c = np.asarray(c, np.float64)
    vals = (((c[4] * pts + c[3]) * pts + c[2]) * pts + c[1]) * pts + c[0]
    bars = sum(abs(c[i]) * pts ** i for i in range(5))
    bad = f > vals + 8 * U * float(horner_bar(c, t)) + 8 * U * bars
    assert not np.any(bad), (list(c), t_max, t, pts[bad][:3])
    return t


def test_quartic_min_against_brute_force():
    rng = np.random.default_rng(2024)
    n = 0
    for i in range(300):
        c = rng.standard_normal(5) * 10.0 ** rng.integers(-3, 4, size=5)
        kind = i % 6
        if kind == 1:
            c[4] = 0.0                                                       # a cubic
        elif kind == 2:
            c[4] = c[3] = 0.0                                                # a parabola
        elif kind == 3:                                                      # two wells inside the interval: (t - a)^2 (t - b)^2 + tilt
            a, b = np.sort(rng.uniform(0.2, 3.0, size=2))
            w = np.polymul(np.polymul([1, -a], [1, -a]), np.polymul([1, -b], [1, -b]))[::-1]
            c = w * 10.0 ** rng.integers(-2, 3) + np.array([rng.standard_normal(), 0.05 * rng.standard_normal(), 0, 0, 0])
        t_max = float(10.0 ** rng.uniform(-2, 1.5)) if kind != 3 else 4.0
        rc, o = raw_min(c, t_max)
        assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
        brute_force(c, t_max, o)
        if c[4] > 0 or (c[4] == 0 and c[3] == 0 and c[2] > 0):
            rc, o = raw_min(c, INF)
            assert rc == 0
            brute_force(c, INF, o)
            n += 1
    assert n > 50


def test_quartic_min_named_cases():
    # two wells of equal depth; a tie in exact arithmetic; with the deeper well on either side
    w = np.polymul(np.polymul([1, -1], [1, -1]), np.polymul([1, -3], [1, -3]))[::-1].astype(np.float64)   # (t - 1)^2 (t - 3)^2, exact integers
    rc, o = raw_min(w, 10.0)
    assert rc == 0 and min(abs(o[0] - 1.0), abs(o[0] - 3.0)) <= 8 * U and abs(o[1]) <= 8 * U * float(horner_bar(w, o[0])) and o[3] == 3
    rc, o = raw_min([0.0, 0.0, 4.0, -4.0, 1.0], 10.0)                        # t^2 (t - 2)^2: 0 at t = 0 and at t = 2, the tie goes to the smaller t
    assert rc == 0 and o[0] == 0.0 and o[1] == 0.0 and o[2] == 0.0 and o[3] == 2 and not np.signbit(o[0])
    rc, o = raw_min(w + np.array([0, 0.5, 0, 0, 0]), 10.0)                    # tilted up to the right: the left well
    assert rc == 0 and abs(o[0] - 1.0) < 0.1 and o[3] == 3
    rc, o = raw_min(w - np.array([0, 0.5, 0, 0, 0]), 10.0)                    # tilted down to the right: the right well
    assert rc == 0 and abs(o[0] - 3.0) < 0.1 and o[3] == 3
    brute_force(w - np.array([0, 0.5, 0, 0, 0]), 10.0, o)
    # a minimum at each endpoint
    rc, o = raw_min([1.0, 2.0, 1.0, 0.0, 1.0], 5.0)                          # increasing on [0, inf)
    assert rc == 0 and o[0] == 0.0 and o[1] == 1.0 and o[2] == 0.0 and o[3] == 0
    rc, o = raw_min([1.0, -2.0, 0.0, 0.0, 0.001], 3.0)                       # decreasing on [0, 3]
    assert rc == 0 and o[0] == 3.0 and o[1] == horner([1.0, -2.0, 0.0, 0.0, 0.001], 3.0) and o[3] == 0
    # a cubic and a parabola; the parabola on [0, inf)
    rc, o = raw_min([0.0, -1.0, 0.0, 1.0 / 3.0, 0.0], 5.0)                   # t^3 / 3 - t: t = 1
    assert rc == 0 and abs(o[0] - 1.0) <= 4 * U and o[3] == 1
    for t_max in (10.0, INF):
        rc, o = raw_min([3.0, -4.0, 2.0, 0.0, 0.0], t_max)                   # 2 (t - 1)^2 + 1
        assert rc == 0 and o[0] == 1.0 and o[1] == 1.0 and o[2] == -2.0 and o[3] == 1
    # all coefficients zero; t_max = 0
    rc, o = raw_min(np.zeros(5), 7.0)
    assert rc == 0 and np.array_equal(o, np.zeros(4)) and not np.signbit(o[0])
    rc, o = raw_min([2.0, -1.0, 0.0, 0.0, 1.0], 0.0)
    assert rc == 0 and o[0] == 0.0 and o[1] == 2.0 and o[2] == 0.0
    # the Python front end
    q = cuadmm_amd.quartic_min([3.0, -4.0, 2.0, 0.0, 0.0], INF)
    assert q == {"t": 1.0, "f": 1.0, "decrease": -2.0, "critical": 1}


def test_quartic_min_refusals():
    lib = cuadmm_amd.load()
    ok = np.array([1.0, -1.0, 1.0, 0.5, 1.0])
    for i in range(5):
        for bad in (np.nan, np.inf, -np.inf):
            c = ok.copy()
            c[i] = bad
            rc, o = raw_min(c, 1.0)
            assert rc == -1 and np.all(np.isnan(o)) and b"quartic_min" in lib.cuadmm_last_error()
    for t_max in (-1.0, -1e-300, np.nan, -np.inf):
        rc, o = raw_min(ok, t_max)
        assert rc == -1 and np.all(np.isnan(o))
    # unbounded below on [0, inf), or not covered by the rule
    for c in ([0, 0, 0, 0, -1.0], [0, 0, 0, 1.0, 0], [0, 0, 0, -1.0, 0], [0, 0, -1.0, 0, 0], [0, -1.0, 0, 0, 0], [0, 1.0, 0, 0, 0], [0, 0, 0, 0, 0],
              [0, 0, 1.0, 1.0, 0]):
        rc, o = raw_min(np.array(c, np.float64), INF)
        assert rc == -1 and np.all(np.isnan(o)) and b"unbounded" in lib.cuadmm_last_error()
    o = np.zeros(4)
    assert lib.cuadmm_quartic_min(None, 1.0, P(o)) == -1 and lib.cuadmm_quartic_min(P(ok), 1.0, None) == -1
    with pytest.raises(cuadmm_amd.CuadmmError):
        cuadmm_amd.quartic_min([0, 0, 0, 0, -1.0], INF)
    with pytest.raises(ValueError, match="quartic_min"):
        cuadmm_amd.quartic_min([1.0, 2.0], 1.0)


def test_the_task_list_is_the_outer_products_own():
    """cuadmm_op_block_outer3 walks the list cuadmm_op_block_outer_plan returns: n = 113 with split_from = 33 is 36 tiles in two workgroups;
    no planner of its own is exported, and the planner's refusal of a split_from <= 32 comes back before any device work"""
    lib = cuadmm_amd.load()
    blk = np.array([113], np.int32)
    n = lib.cuadmm_op_block_outer_plan(P(blk), 1, 5, 33, None, None, 0)
    t = np.full(4 * n, -9, np.int32)
    assert n == 8 and lib.cuadmm_op_block_outer_plan(P(blk), 1, 5, 33, None, P(t), n) == n
    assert t.reshape(8, 4).tolist() == [[0, w, 32, 4] for w in range(4)] + [[0, 32 + w, 36, 4] for w in range(4)]
    assert hasattr(lib, "cuadmm_op_block_outer3") and not hasattr(lib, "cuadmm_op_block_outer3_plan")
    ranks, L = np.array([5], np.int32), np.ones(113 * 5)
    dummy = C.c_void_p(4096)                                                 # never dereferenced: the refusals come first
    assert lib.cuadmm_op_block_outer3(P(L), P(L), P(ranks), P(blk), 1, 5, 32, dummy, dummy, dummy, None) == -1
    assert lib.cuadmm_op_block_outer3(P(L), None, P(ranks), P(blk), 1, 5, 33, dummy, dummy, dummy, None) == -1
    assert lib.cuadmm_op_block_outer3(P(L), P(L), P(np.array([6], np.int32)), P(blk), 1, 5, 33, dummy, dummy, dummy, None) == -1


BLK, M = [3, 6, -2, 5], 7
RANKS = (2, 3, 0, 5)


def _factors(rng):
    return [rng.integers(-2048, 2049, size=(max(n, 0), r if n > 0 else 0)) / 1024.0 for n, r in zip(BLK, RANKS)]


@pytest.mark.parametrize("sigma", [0.0, 0.7])
def test_the_twins_quartic_is_lowrank_grads_f_along_the_line(sigma):
    """the twin's c0 .. c4 evaluated at t against the twin of cuadmm_lowrank_grad at L + t D (dyadic L, D, t: every L + t D is exact).  Both
    are sums of at most vec_len + m + 16 products in longdouble (unit v = eps / 2) of terms bounded by the chains."""
    fx = make_opt_fixture(BLK, M, 3)
    rng = np.random.default_rng(5)
    X = rng.integers(-2048, 2049, size=fx.L) / 1024.0
    y = rng.standard_normal(fx.m)
    Ls, Ds = _factors(rng), _factors(rng)
    tw = twin(fx, X, Ls, Ds, y, sigma)
    v = LD(np.finfo(LD).eps) / 2
    Kt = fx.L + fx.m + 16
    for t in (-1.0, 0.5, 1.0, 2.0):
        g = grad_twin(fx, X, [L + t * D for L, D in zip(Ls, Ds)], y, sigma)
        assert abs(horner(tw["c"], t, LD) - g["f"]) <= 2 * Kt * v * horner_bar(tw["cb"], t)
    g0 = grad_twin(fx, X, Ls, y, sigma)
    assert abs(tw["c"][0] - g0["f"]) <= Kt * v * tw["cb"][0] and np.all(np.abs(tw["r"] - g0["r"]) <= Kt * v * tw["rb"])
    slope = sum(np.sum(G * D.astype(LD)) for G, D in zip(g0["G"], Ds))      # c1 = <G, D>
    assert abs(tw["c"][1] - slope) <= 4 * Kt * v * tw["cb"][1] and abs(slope) > 1e6 * Kt * v * tw["cb"][1]


def test_python_packing_and_refusals_need_no_device():
    rng = np.random.default_rng(9)
    Ls, Ds = _factors(rng), _factors(rng)
    Lv, Dv, ranks, rmax, yv, sigma, t_max = lowrank_line_args(BLK, M, Ls, Ds, None, 0.5, 2)
    assert rmax == 5 and ranks.tolist() == [2, 3, 0, 5] and yv is None and sigma == 0.5 and t_max == 2.0
    assert Lv.size == Dv.size == lowrank_size(BLK, 5) and np.array_equal(Dv[:6], Ds[0].T.ravel())
    assert lowrank_line_args(BLK, M, Ls, Ds, None, 0.5, INF)[6] == INF
    for sig in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="lowrank_line: sigma"):
            lowrank_line_args(BLK, M, Ls, Ds, None, sig, 1.0)
    with pytest.raises(ValueError, match="lowrank_line: t_max"):
        lowrank_line_args(BLK, M, Ls, Ds, None, 0.5, np.nan)
    with pytest.raises(ValueError, match="lowrank_line: y has"):
        lowrank_line_args(BLK, M, Ls, Ds, np.zeros(M + 1), 0.5, 1.0)
    other = [d.copy() for d in Ds]
    other[1] = np.zeros((6, 2))
    with pytest.raises(ValueError, match="lowrank_line: D has the ranks"):
        lowrank_line_args(BLK, M, Ls, other, None, 0.5, 1.0)
    other[1] = np.zeros((5, 3))
    for arg in (other, Ds[:3]):
        with pytest.raises(ValueError, match="lowrank_line"):
            lowrank_line_args(BLK, M, Ls, arg, None, 0.5, 1.0)
