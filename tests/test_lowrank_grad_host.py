"""cuadmm_lowrank_grad without a device: the longdouble twin against itself, and the Python front end's packing and refusals
(tests/_lowrank_grad_twin.py; cuadmm_amd/solver.py: lowrank_grad_args, pack_lowrank, unpack_lowrank)."""
import numpy as np
import pytest

from cuadmm_amd.solver import lowrank_grad_args, pack_lowrank, unpack_lowrank
from tests._block_mult_twin import LD, loffs, lowrank_size, offsets
from tests._lower_bound_twin import make_opt_fixture
from tests._lowrank_grad_twin import five_point, inner, twin

BLK, M = [3, 6, -2, 5], 7
RANKS = (2, 3, 0, 5)


def _factors(rng, blk=BLK, ranks=RANKS):
    """entries that are multiples of 2^-10 in [-2, 2]: with h = 2^-3 every L + t D of the five-point formula is exact in double"""
    return [rng.integers(-2048, 2049, size=(max(n, 0), r if n > 0 else 0)) / 1024.0 for n, r in zip(blk, ranks)]


@pytest.mark.parametrize("sigma", [0.0, 0.7])
def test_five_point_identity_of_the_twin(sigma):
    """t -> f(L + t D) is a quartic, so the five-point formula gives <G(L), D> exactly.  The twin's own rounding: every number it forms is a
    sum of at most vec_len + m + n + 16 products in longdouble (unit v = eps / 2), so f is within that many v of fbar at each of the four
    points -- they enter the formula with weights 1 + 8 + 8 + 1 over 12 h -- and <G, D> within as many v of <Gbar, |D|>."""
    fx = make_opt_fixture(BLK, M, 3)
    rng = np.random.default_rng(5)
    X = rng.integers(-2048, 2049, size=fx.L) / 1024.0                       # (X + t d is exact too)
    y = rng.standard_normal(fx.m)
    Ls, Ds = _factors(rng), _factors(rng)
    h = 2.0 ** -3
    at = lambda t: twin(fx, X, [L + t * D for L, D in zip(Ls, Ds)], y, sigma)
    pts = [at(t) for t in (-2 * h, -h, h, 2 * h)]
    t0 = at(0.0)
    v = LD(np.finfo(LD).eps) / 2
    Kt = fx.L + fx.m + max(BLK) + 16
    lhs, rhs = five_point([p["f"] for p in pts], h), inner(t0["G"], Ds)
    tol = 18 / (12 * LD(h)) * Kt * v * max(p["fb"] for p in pts) + Kt * v * inner(t0["Gb"], [np.abs(D) for D in Ds])
    print("five-point %.18Lg, <G, D> %.18Lg, difference %.3Lg, tolerance %.3Lg" % (lhs, rhs, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol
    assert abs(rhs) > 1e6 * tol                                             # (the identity is not met by two zeros)
    # the free slices of S^ are the gradient with respect to the free part of x: one more five-point check along a direction there
    off = offsets(BLK)
    d = np.zeros(fx.L)
    d[off[2]:off[3]] = rng.integers(-2048, 2049, size=2) / 1024.0
    pts = [twin(fx, X + t * d, Ls, y, sigma) for t in (-2 * h, -h, h, 2 * h)]
    lhs, rhs = five_point([p["f"] for p in pts], h), np.sum(t0["Sh"] * d.astype(LD))
    assert abs(lhs - rhs) <= 18 / (12 * LD(h)) * Kt * v * max(p["fb"] for p in pts) + Kt * v * np.sum(t0["Sb"] * np.abs(d))


def test_python_packing_and_unpacking():
    rng = np.random.default_rng(9)
    Ls = _factors(rng)
    Lv, ranks, rmax, yv, sigma = lowrank_grad_args(BLK, M, Ls, None, 0.5)
    assert rmax == 5 and ranks.tolist() == [2, 3, 0, 5] and yv is None and sigma == 0.5 and Lv.size == lowrank_size(BLK, 5)
    lo = loffs(BLK, rmax)
    for k, n in enumerate(BLK):
        if n > 0:
            r = Ls[k].shape[1]
            assert np.array_equal(Lv[lo[k]:lo[k] + n * r], Ls[k].T.ravel())
            assert np.all(Lv[lo[k] + n * r:lo[k + 1]] == 0.0)
    back = unpack_lowrank(BLK, ranks, rmax, Lv)
    assert [b.shape for b in back] == [(3, 2), (6, 3), (0, 0), (5, 5)]
    assert all(np.array_equal(a, b) for a, b in zip(back, Ls))
    # the same buffer as the twins' pack, and pack_lowrank's own rmax
    assert np.array_equal(Lv, pack_lowrank(BLK, Ls)[0])
    # a y is passed on as float64 of con_num entries; every rank 0: rmax = 1, a buffer of zeros
    y = lowrank_grad_args(BLK, M, Ls, list(range(M)), 0)[3]
    assert y.dtype == np.float64 and y.tolist() == list(range(M))
    Lv, ranks, rmax = lowrank_grad_args(BLK, M, [np.zeros((max(n, 0), 0)) for n in BLK], None, 0.0)[:3]
    assert rmax == 1 and not ranks.any() and not Lv.any()


def test_python_refusals_need_no_device():
    rng = np.random.default_rng(11)
    Ls = _factors(rng)
    for sigma in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="lowrank_grad: sigma"):
            lowrank_grad_args(BLK, M, Ls, None, sigma)
    for y in (np.zeros(M - 1), np.zeros(M + 1), np.zeros(0)):
        with pytest.raises(ValueError, match="lowrank_grad: y has"):
            lowrank_grad_args(BLK, M, Ls, y, 0.0)
    bad_rows, too_wide = [m.copy() for m in Ls], [m.copy() for m in Ls]
    bad_rows[1] = np.zeros((5, 2))
    too_wide[0] = np.zeros((3, 4))
    for arg in (bad_rows, too_wide, Ls[:3], [m.ravel() for m in Ls]):
        with pytest.raises(ValueError, match="lowrank_grad"):
            lowrank_grad_args(BLK, M, arg, None, 0.0)
