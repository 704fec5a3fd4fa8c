"""The quartic along a line in factor space on the GPU (include/cuadmm_amd.h: cuadmm_lowrank_line, cuadmm_op_block_outer3,
cuadmm_op_lrl_sums; csrc/lowrank_line.h; DESIGN.md, "Line search along factor steps"): the two new kernels through their op hooks, then the
solver entry against the longdouble twin of tests/_lowrank_line_twin.py, its ties to cuadmm_lowrank_grad, the solve that continues bit
for bit, the refusals, the front ends and the descent driver.

Tolerances, none of them measured (u = 2^-53): every output within gamma(K) times its absolute-value chain, K counted from the code launch
by launch in the twin's docstring (constants()).  On fixture A with ranks (3, 20, 6, 0, 9): c = 11218, R = 20, m = 40, vec_len = 11218, so
K_r = K_q = 11254, K_p = 11274, K_cx = 11254, K_cx1 = 11274, K_c0 = 22816, K_c1 = 22837, K_c2 = 22858, K_c3 = 22836, K_c4 = 22816.
Measured share of the bound on the MI355X (largest err / bound over the entries): see NOTEBOOK.md, Round 21."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd.devbuf import Dev
from tests._block_mult_twin import LD, loffs, lowrank_size, offsets, pack
from tests._infeas_twin import Fixture
from tests._lower_bound_twin import make_opt_fixture
from tests._lowrank_grad_twin import constants as grad_constants, gamma, inner, twin as grad_twin
from tests._lowrank_line_twin import U, constants, horner, horner_bar, outer3, twin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
SQ2 = 1.4142135623730951                       # kLoSqrt2
BLK_A, M_A = [3, 20, 70, -2, 130], 40          # the fixture of tests/test_gpu_lowrank_grad.py
RANKS = (3, 20, 6, 0, 9)
RMAX = 20
INFO = ("pobj", "dobj", "errRp", "errRd", "relgap", "sig", "bscale", "Cscale")
INF = float("inf")
_fx = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def share(err, bound):
    err, bound = np.atleast_1d(np.asarray(err, LD)), np.atleast_1d(np.asarray(bound, LD))
    return float(np.max(err / np.maximum(bound, np.finfo(LD).tiny))) if err.size else 0.0


# ---- 1. the three outer products ------------------------------------------------------------------------------------------
BLK_O = [1, 2, 15, 16, 17, -3, 31, 32, 33, 48, 65]       # an unconstrained block between two of them
RANKS_O = [1, 0, 3, 4, 5, 9, 31, 1, 4, 5, 65]            # 0, 1, 3, 4, 5 and n spread over the blocks (the free block's is ignored)
SENT = -7.25


def outer3_dev(blk, Ls, Ds, rmax, split_from=0, poison=np.nan):
    lib = cuadmm_amd.load()
    Lv, ranks = pack(blk, Ls, rmax, poison)
    Dv, _ = pack(blk, Ds, rmax, poison)
    off = offsets(blk)
    d = [Dev(np.full(off[-1], SENT)) for _ in range(3)]
    b = np.asarray(blk, np.int32)
    rc = lib.cuadmm_op_block_outer3(P(Lv), P(Dv), P(ranks), P(b), b.size, rmax, split_from, d[0].ptr, d[1].ptr, d[2].ptr, None)
    assert rc == 0, lib.cuadmm_last_error()
    return [v.get() for v in d]


def outer_dev(blk, Ls, rmax):
    lib = cuadmm_amd.load()
    Lv, ranks = pack(blk, Ls, rmax)
    d = Dev(np.full(offsets(blk)[-1], SENT))
    b = np.asarray(blk, np.int32)
    assert lib.cuadmm_op_block_outer(P(Lv), P(ranks), P(b), b.size, rmax, d.ptr, None) == 0, lib.cuadmm_last_error()
    return d.get()


def op_factors(blk, ranks, seed, integers=False):
    rng = np.random.default_rng(seed)
    gen = (lambda s: rng.integers(-9, 10, size=s).astype(np.float64)) if integers else rng.standard_normal
    return [gen((max(n, 0), r if n > 0 else 0)) for n, r in zip(blk, ranks)]


@pytest.mark.parametrize("blk,ranks,rmax,split", [(BLK_O, RANKS_O, 65, 0), ([113], [5], 5, 33), ([113, -2, 40], [113, 0, 7], 113, 33)])
def test_outer3(blk, ranks, rmax, split):
    Ls, Ds = op_factors(blk, ranks, 1), op_factors(blk, ranks, 2)
    x = outer3_dev(blk, Ls, Ds, rmax, split)
    assert same_bits(x[0], outer_dev(blk, Ls, rmax)) and same_bits(x[2], outer_dev(blk, Ds, rmax))
    off = offsets(blk)
    sh = 0.0
    for k, n in enumerate(blk):
        sl = slice(off[k], off[k + 1])
        if n < 0:
            assert all(same_bits(v[sl], np.full(-n, SENT)) for v in x)      # the sentinel stays in all three
            continue
        r = ranks[k]
        if r == 0:
            assert all(same_bits(v[sl], np.zeros(off[k + 1] - off[k])) for v in x)      # + 0.0
            continue
        ref, bar = outer3(Ls[k], Ds[k])
        for j, K in ((0, r + 4), (1, 2 * r + 4), (2, r + 4)):
            err, bound = np.abs(x[j][sl].astype(LD) - ref[j]), K * LD(U) * bar[j]
            sh = max(sh, share(err, bound))
            assert np.all(err <= bound), (k, j)
    print("outer3 share of the bound: %.2e" % sh)
    # D -> -D: x1 changes sign bit for bit, x0 and x2 keep their bits; another poison behind the columns: the same bits
    neg = outer3_dev(blk, Ls, [-D for D in Ds], rmax, split, poison=np.inf)
    psd = np.concatenate([np.arange(off[k], off[k + 1]) for k, n in enumerate(blk) if n > 0])
    assert same_bits(neg[0], x[0]) and same_bits(neg[2], x[2]) and np.array_equal(neg[1][psd], -x[1][psd])
    nz = psd[x[1][psd] != 0]
    assert nz.size > psd.size // 2 and same_bits(neg[1][nz], -x[1][nz])
    assert all(same_bits(a, b) for a, b in zip(outer3_dev(blk, Ls, Ds, rmax, split, poison=1e300), x))


def test_outer3_is_exact_on_integers():
    blk, ranks = BLK_O, RANKS_O
    Ls, Ds = op_factors(blk, ranks, 3, True), op_factors(blk, ranks, 4, True)
    x = outer3_dev(blk, Ls, Ds, 65)
    off = offsets(blk)
    for k, n in enumerate(blk):
        if n <= 0:
            continue
        ii, jj = np.tril_indices(n)
        for j, M in enumerate((Ls[k] @ Ls[k].T, Ls[k] @ Ds[k].T + Ds[k] @ Ls[k].T, Ds[k] @ Ds[k].T)):
            want = np.where(ii == jj, M[ii, jj], SQ2 * M[ii, jj]) + 0.0
            assert same_bits(x[j][off[k]:off[k + 1]] + 0.0, want), (k, j)


# ---- 2. the quartic sums --------------------------------------------------------------------------------------------------
def lrl_sums(ax, b, normA, y, bscale, Cscale, shift):
    """shift = 1: every array a view that starts 8 bytes behind a 16-byte boundary"""
    m = ax[0].size

    def view(a):
        base = np.zeros(m + 3)
        at = (((base.ctypes.data >> 3) & 1) + shift) % 2
        v = base[at:at + m]
        v[:] = a
        assert ((v.ctypes.data >> 3) & 1) == shift
        return v
    ins = [view(a) for a in (*ax, b, normA, y)]
    outs = [view(np.full(m, np.nan)) for _ in range(3)]
    o = np.full(9, np.nan)
    rc = cuadmm_amd.load().cuadmm_op_lrl_sums(m, *[P(a) for a in ins], bscale, Cscale, *[P(a) for a in outs], P(o))
    assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
    assert not any(np.isnan(a).any() for a in outs) and not np.isnan(o).any()
    return outs, o


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_quartic_sums(m, shift):
    rng = np.random.default_rng(1000 * m + shift)
    ax = [rng.standard_normal(m) * np.exp(rng.uniform(-2, 2, size=m)) for _ in range(3)]
    b, y = (rng.standard_normal(m) * np.exp(rng.uniform(-2, 2, size=m)) for _ in range(2))
    normA = rng.uniform(1.0, 3.0, size=m)
    bscale, Cscale = 1 + 2.3 * rng.random(), 1 + 5.1 * rng.random()
    (r, p, q), o = lrl_sums(ax, b, normA, y, bscale, Cscale, shift)
    yt = np.full(m, np.nan)
    r_lg, o2 = np.full(m, np.nan), np.full(2, np.nan)
    assert cuadmm_amd.load().cuadmm_op_lrg_multiplier(m, P(ax[0]), P(b), P(normA), P(y), bscale, Cscale, 0.5, P(yt), P(r_lg), P(o2)) == 0
    rs = ax[0] - b
    assert same_bits(r, r_lg) and same_bits(r, (normA * rs) * bscale)
    assert same_bits(p, (normA * ax[1]) * bscale) and same_bits(q, (normA * ax[2]) * bscale)      # (xunit = 1: its product is exact)
    l = lambda a: np.asarray(a).astype(LD)
    unit = LD(bscale * Cscale)
    terms = [l(y) * l(rs) * unit, l(y) * l(ax[1]) * unit, l(y) * l(ax[2]) * unit, l(r) * l(r), l(r) * l(p), l(p) * l(p), l(r) * l(q), l(p) * l(q), l(q) * l(q)]
    sh = 0.0
    for j, t in enumerate(terms):       # the products of the rounded vectors: one rounding each (and the unit's two) lies inside the slack of 8
        err, bound = abs(LD(o[j]) - np.sum(t)), (m / 256 + 264) * LD(U) * np.sum(np.abs(t))
        sh = max(sh, share(err, bound))
        assert err <= bound, (j, float(err), float(bound))
    print("quartic sums share of the bound: %.2e" % sh)
    again = lrl_sums(ax, b, normA, y, bscale, Cscale, shift)
    assert all(same_bits(u, v) for u, v in zip(again[0], (r, p, q))) and same_bits(again[1], o)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_quartic_sums_are_exact_on_integers(m, shift):
    rng = np.random.default_rng(m)
    ax = [rng.integers(-9, 10, size=m).astype(np.float64) for _ in range(3)]
    b, y = (rng.integers(-9, 10, size=m).astype(np.float64) for _ in range(2))
    normA = 2.0 ** rng.integers(0, 3, size=m)
    bscale, Cscale = 4.0, 2.0
    (r, p, q), o = lrl_sums(ax, b, normA, y, bscale, Cscale, shift)
    rs = ax[0] - b
    wr, wp, wq = normA * rs * bscale, normA * ax[1] * bscale, normA * ax[2] * bscale
    assert same_bits(r, wr) and same_bits(p, wp) and same_bits(q, wq)
    want = [8 * np.sum(y * rs), 8 * np.sum(y * ax[1]), 8 * np.sum(y * ax[2]), np.sum(wr * wr), np.sum(wr * wp), np.sum(wp * wp), np.sum(wr * wq),
            np.sum(wp * wq), np.sum(wq * wq)]
    assert np.array_equal(o, np.array(want, np.float64))


# ---- 3. the solver entry --------------------------------------------------------------------------------------------------
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


def factors(seed, ranks=RANKS, dyadic=False, blk=BLK_A):
    rng = np.random.default_rng(seed)
    if dyadic:                                                              # multiples of 2^-10 in [-2, 2]
        return [rng.integers(-2048, 2049, size=(max(n, 0), r if n > 0 else 0)) / 1024.0 for n, r in zip(blk, ranks)]
    return [rng.standard_normal((max(n, 0), r if n > 0 else 0)) for n, r in zip(blk, ranks)]


def raw(s, Lv, Dv, ranks, rmax, y, sigma, t_max, coef=True, out=True, m=M_A, nb=len(BLK_A)):
    """(rc, coef5, r, p, q, out8, per_block) of cuadmm_lowrank_line; the outputs pre-filled with NaN"""
    c = np.full(5, np.nan) if coef else None
    r, p, q = (np.full(m, np.nan) for _ in range(3))
    o = np.full(8, np.nan) if out else None
    pb = np.full(4 * nb, np.nan)
    rc = cuadmm_amd.load().cuadmm_lowrank_line(s._h, P(Lv), P(Dv), P(ranks), rmax, P(y), float(sigma), float(t_max), P(c), P(r), P(p), P(q), P(o), P(pb))
    return rc, c, r, p, q, o, pb


def check_against_twin(tw, K, ln, what):
    l = lambda a: np.asarray(a).astype(LD)
    sh = {}
    for name, got, ref, bound in (("r", ln["r"], tw["r"], gamma(K["r"]) * tw["rb"]), ("p", ln["p"], tw["p"], gamma(K["p"]) * tw["pb"]),
                                  ("q", ln["q"], tw["q"], gamma(K["q"]) * tw["qb"]),
                                  ("per_block", ln["per_block"][:, :3], tw["pbk"], gamma(np.array([K["cx"], K["cx1"], K["cx"]])) * tw["pbkb"])):
        err = np.abs(l(got) - ref)
        sh[name] = share(err, bound)
        assert np.all(err <= bound), (what, name, sh[name])
    for j in range(5):
        err, bound = abs(LD(ln["coef"][j]) - tw["c"][j]), gamma(K["c%d" % j]) * tw["cb"][j]
        sh["c%d" % j] = share(err, bound)
        assert err <= bound, (what, "c%d" % j, sh["c%d" % j])
    assert abs(LD(ln["pnorm"]) - np.sqrt(tw["p"] @ tw["p"])) <= gamma(2 * K["p"] + M_A + 268) * np.sqrt(tw["pb"] @ tw["pb"])
    assert abs(LD(ln["qnorm"]) - np.sqrt(tw["q"] @ tw["q"])) <= gamma(2 * K["q"] + M_A + 268) * np.sqrt(tw["qb"] @ tw["qb"])
    assert ln["per_block"][:, 3].tolist() == [0.0 if n > 0 else 2.0 for n in BLK_A]
    print(what, "share of the bound:", ", ".join("%s %.2e" % kv for kv in sorted(sh.items())))


def coef_bound(tw, K, t):
    """what the five coefficients' roundings and Horner's scheme (8 u) allow the quartic's value at t"""
    return sum(gamma(K["c%d" % j]) * tw["cb"][j] * abs(LD(t)) ** j for j in range(5)) + 8 * LD(U) * horner_bar(tw["cb"], t)


def start():
    fx = fixture()
    rng = np.random.default_rng(41)
    s = solver(fx, rng.standard_normal(fx.L))
    return fx, s, s.X, rng.standard_normal(fx.m), 0.7


def test_against_the_twin_and_lowrank_grad():
    fx, s, X0, y, sigma = start()
    Ls, Ds = factors(43, dyadic=True), factors(44, dyadic=True)
    Lv, ranks = pack(BLK_A, Ls, RMAX)                                       # NaN in every column that must not be read
    Dv, _ = pack(BLK_A, Ds, RMAX)
    assert np.isnan(Lv).any() and np.isnan(Dv).any()
    rc, c, r, p, q, o, pb = raw(s, Lv, Dv, ranks, RMAX, y, sigma, INF)
    assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
    assert not any(np.isnan(v).any() for v in (c, r, p, q, o, pb))
    ln = s.lowrank_line(Ls, Ds, y, sigma)
    assert same_bits(ln["coef"], c) and same_bits(ln["r"], r) and same_bits(ln["p"], p) and same_bits(ln["q"], q) and same_bits(ln["per_block"].ravel(), pb)
    assert same_bits([ln[k] for k in ("t", "f", "decrease", "pnorm", "qnorm")], o[:5]) and ln["critical"] == o[5]
    K, Kg = constants(fx, RANKS), grad_constants(fx, RANKS)
    tw = twin(fx, X0, Ls, Ds, y, sigma)
    check_against_twin(tw, K, ln, "fresh solver:")
    assert o[6] > 0 and o[7] >= 8 * (3 * fx.L + 7 * fx.m + 2 * lowrank_size(BLK_A, RMAX))
    # the minimiser is cuadmm_quartic_min's
    qm = cuadmm_amd.quartic_min(c, INF)
    assert same_bits([qm["t"], qm["f"], qm["decrease"]], o[:3]) and qm["critical"] == o[5]
    # t_max <= 0: coefficients only; the outputs that may be null
    rc0, c0, r0, _, _, o0, _ = raw(s, Lv, Dv, ranks, RMAX, y, sigma, 0.0)
    assert rc0 == 0 and same_bits(c0, c) and same_bits(r0, r) and same_bits(o0[:6], [0.0, c[0], 0.0, o[3], o[4], 0.0])
    o1 = np.full(8, np.nan)
    assert cuadmm_amd.load().cuadmm_lowrank_line(s._h, P(Lv), P(Dv), P(ranks), RMAX, P(y), sigma, -1.0, P(c0), None, None, None, P(o1), None) == 0
    assert same_bits(o1[:6], o0[:6])
    # lowrank_grad at the same L: r bit for bit; c0 = f and c1 = <G, D> within the sum of the two bounds
    g = s.lowrank_grad(Ls, y, sigma)
    gt = grad_twin(fx, X0, Ls, y, sigma)
    assert same_bits(g["r"], r)
    assert abs(LD(c[0]) - LD(g["f"])) <= gamma(K["c0"]) * tw["cb"][0] + gamma(Kg["f"]) * gt["fb"]
    nG = sum(G.size for G in g["G"])
    slope = sum(float(np.cumsum((G * D).T.ravel())[-1]) for G, D in zip(g["G"], Ds) if G.size)
    allow = gamma(K["c1"]) * tw["cb"][1] + gamma(Kg["G"] + nG + 1) * inner(gt["Gb"], [np.abs(D) for D in Ds])
    print("c1 %.15e, <G, D> %.15e, difference %.3e, allowance %.3e" % (c[1], slope, abs(c[1] - slope), float(allow)))
    assert abs(LD(c[1]) - LD(slope)) <= allow and abs(slope) > 100 * allow
    # the quartic is the function: L + t D is exact for these dyadic factors
    for t in (-1.0, 0.5, 1.0, 2.0):
        Lt = [L + t * D for L, D in zip(Ls, Ds)]
        assert all(np.array_equal((a - b) / t, d) for a, b, d in zip(Lt, Ls, Ds))
        ft = s.lowrank_grad(Lt, y, sigma)["f"]
        allow = coef_bound(tw, K, t) + gamma(Kg["f"]) * grad_twin(fx, X0, Lt, y, sigma)["fb"]
        print("t = %4.1f: f %.15e, quartic %.15e, difference %.3e, allowance %.3e" % (t, ft, horner(c, t), abs(ft - horner(c, t)), float(allow)))
        assert abs(LD(ft) - LD(horner(c, t))) <= allow
    # D -> -D: c1 and c3 change sign bit for bit, c0, c2, c4 keep their bits; D = 0: c1 .. c4 = + 0.0 and t* = 0
    neg = s.lowrank_line(Ls, [-D for D in Ds], y, sigma, 1.0)["coef"]
    assert same_bits(neg, c * np.array([1, -1, 1, -1, 1.0])) and c[1] != 0 and c[3] != 0
    z = s.lowrank_line(Ls, [np.zeros(D.shape) for D in Ds], y, sigma, 1.0)
    assert same_bits(z["coef"], [c[0], 0.0, 0.0, 0.0, 0.0]) and same_bits([z["t"], z["decrease"]], [0.0, 0.0]) and z["f"] == c[0]
    assert same_bits(s.X, X0)                                               # the resident X keeps its bits


def dyadic_fixture():
    """Small integers everywhere and powers of two for every scale: A has one entry +-2^e per row on a diagonal slot of a PSD block or on a
    free slot (no sqrt(2) enters), ||b / normA|| = ||C|| = 3 so that bscale = Cscale = 4; C on diagonal and free slots."""
    blk = [4, -3, 6]
    off = offsets(blk)
    diag = lambda k, i: int(off[k] + i * (i + 1) // 2 + i)
    slots = [diag(0, 0), diag(0, 2), off[1] + 1, diag(2, 1), diag(2, 5), diag(0, 3)]
    A = np.zeros((len(slots), off[-1]))
    for i, (sl, e) in enumerate(zip(slots, (1.0, -2.0, 4.0, 1.0, -1.0, 2.0))):
        A[i, sl] = e
    b = np.array([1.0, 4.0, 0.0, -2.0, 0.0, 0.0])                           # b / normA = (1, 2, 0, -2, 0, 0): norm 3
    Cv = np.zeros(off[-1])
    Cv[diag(0, 1)], Cv[off[1]], Cv[diag(2, 5)] = 1.0, -2.0, 2.0            # norm 3
    return Fixture(blk, A, b, Cv), blk


def test_dyadic_fixture_is_exact():
    fx, blk = dyadic_fixture()
    rng = np.random.default_rng(7)
    X0 = rng.integers(-3, 4, size=fx.L).astype(np.float64)
    s = solver(fx, X0)
    ranks = (2, 0, 3)
    Ls = [rng.integers(-3, 4, size=(max(n, 0), r if n > 0 else 0)).astype(np.float64) for n, r in zip(blk, ranks)]
    Ds = [rng.integers(-3, 4, size=(max(n, 0), r if n > 0 else 0)).astype(np.float64) for n, r in zip(blk, ranks)]
    y = rng.integers(-3, 4, size=fx.m).astype(np.float64)
    sigma = 2.0
    ln = s.lowrank_line(Ls, Ds, y, sigma, 0.0)
    Xr = s.X                                                                # what the solver holds after init: the free slice of x0 is its
    assert np.array_equal(Xr * 1024, np.round(Xr * 1024))                   # (small dyadic numbers, as every other operand)
    tw = twin(fx, Xr, Ls, Ds, y, sigma)                                     # so the longdouble values are the exact ones
    assert all(float(v) * 2 ** 20 == int(float(v) * 2 ** 20) for v in tw["c"])
    assert np.array_equal(ln["coef"], tw["c"].astype(np.float64)) and np.array_equal(ln["r"], tw["r"].astype(np.float64))
    assert np.array_equal(ln["p"], tw["p"].astype(np.float64)) and np.array_equal(ln["q"], tw["q"].astype(np.float64))
    assert np.any(ln["coef"][1:] != 0)


def _traj(s):
    return [s.info_arr(k).copy() for k in INFO] + [s.X, s.y, s.S]


def test_behind_a_solve():
    """a: 30 iterations, the call on the pending scaled state, 30 more; b: the same without the call; c: 30 iterations, the call, the
    getters; d: 30 iterations and the getters, which the twin is evaluated at and which a fresh solver e is given through set_XyS."""
    fx = fixture()
    a, b, c, d = (solver(fx) for _ in range(4))
    for s in (a, b, c, d):
        s.solve(30, 0.0)
    Ls, Ds = factors(61), factors(62)
    sigma = 0.7
    la, lc = a.lowrank_line(Ls, Ds, None, sigma), c.lowrank_line(Ls, Ds, None, sigma)
    assert same_bits(la["coef"], lc["coef"]) and same_bits(la["t"], lc["t"])
    assert same_bits(lc["r"], c.lowrank_grad(Ls, None, sigma)["r"])
    K = constants(fx, RANKS)
    tw = twin(fx, d.X, Ls, Ds, d.y, sigma)
    check_against_twin(tw, K, lc, "behind a solve:")
    for u, v in zip((c.X, c.y, c.S), (d.X, d.y, d.S)):
        assert same_bits(u, v)
    e = solver(fx)
    e.set_XyS(X=d.X, y=d.y, S=d.S)
    le = e.lowrank_line(Ls, Ds, None, sigma)
    for j in range(5):
        assert abs(LD(le["coef"][j]) - LD(lc["coef"][j])) <= 2 * gamma(K["c%d" % j]) * tw["cb"][j], j
    for s in (a, b):
        s.solve(30, 0.0, if_first=False)
    for u, v in zip(_traj(a), _traj(b)):
        assert same_bits(u, v)
    assert a.info_iter_num == b.info_iter_num == 30


def status_of(s):
    st = s.status()
    return {k: st[k] for k in st if k not in ("ms", "check_ms")}


def test_refusals_leave_the_solver_as_it_was():
    fx = fixture()
    lib = cuadmm_amd.load()
    a, b = solver(fx), solver(fx)
    for s in (a, b):
        s.solve(20, 0.0)
    Ls, Ds = factors(71), factors(72)
    Lv, ranks = pack(BLK_A, Ls, RMAX)
    Dv, _ = pack(BLK_A, Ds, RMAX)
    Dz = np.where(np.isnan(Dv), Dv, 0.0)
    y = np.random.default_rng(73).standard_normal(fx.m)
    lo = loffs(BLK_A, RMAX)

    def with_rank(k, r):
        q = ranks.copy()
        q[k] = r
        return q

    def with_entry(v, k, col, row, x):
        q = v.copy()
        q[lo[k] + col * BLK_A[k] + row] = x
        return q

    def refused(s):
        for L_, D_, ranks_, rmax_, y_, sigma_, t_ in ((Lv, Dv, ranks, RMAX, y, -0.5, 1.0), (Lv, Dv, ranks, RMAX, y, np.nan, 1.0), (Lv, Dv, ranks, RMAX, None, np.inf, 1.0),
                                                      (Lv, Dv, ranks, 0, y, 0.7, 1.0), (Lv, Dv, ranks, 8193, y, 0.7, 1.0), (Lv, Dv, None, RMAX, y, 0.7, 1.0),
                                                      (Lv, Dv, with_rank(1, -1), RMAX, y, 0.7, 1.0), (Lv, Dv, with_rank(2, 21), RMAX, y, 0.7, 1.0),
                                                      (Lv, Dv, with_rank(0, 4), RMAX, y, 0.7, 1.0), (None, Dv, ranks, RMAX, y, 0.7, 1.0),
                                                      (Lv, None, ranks, RMAX, y, 0.7, 1.0), (with_entry(Lv, 2, 5, 69, np.nan), Dv, ranks, RMAX, y, 0.7, 1.0),
                                                      (Lv, with_entry(Dv, 2, 5, 69, np.nan), ranks, RMAX, y, 0.7, 1.0),
                                                      (Lv, with_entry(Dv, 4, 0, 0, np.inf), ranks, RMAX, None, 0.7, 1.0),
                                                      (Lv, Dv, ranks, RMAX, np.where(np.arange(fx.m) == 7, np.nan, y), 0.7, 1.0),
                                                      (Lv, Dv, ranks, RMAX, y, 0.7, np.nan),
                                                      (Lv, Dz, ranks, RMAX, y, 0.7, INF)):      # D = 0: a constant, which t_max = inf is refused for
            rc, c, r, p, q, o, pb = raw(s, L_, D_, ranks_, rmax_, y_, sigma_, t_)
            assert rc == -1 and all(np.all(np.isnan(v)) for v in (c, r, p, q, o, pb)), (rmax_, sigma_, t_)      # CUADMM_ERR_INVALID, outputs untouched
            assert b"lowrank_line" in lib.cuadmm_last_error() or b"quartic_min" in lib.cuadmm_last_error()
        assert raw(s, Lv, Dv, ranks, RMAX, y, 0.7, 1.0, coef=False)[0] == -1 and raw(s, Lv, Dv, ranks, RMAX, y, 0.7, 1.0, out=False)[0] == -1
    assert np.isnan(Dv[lo[2] + 6 * 70])                                     # a NaN in a column that is not read is no reason to refuse
    refused(a)                                                              # on the pending scaled state: it must stay pending
    assert status_of(a) == status_of(b)
    for s in (a, b):
        s.solve(5, 0.0, if_first=False)
    refused(a)
    ta, tb = _traj(a), _traj(b)
    for u, v in zip(ta, tb):
        assert same_bits(u, v)
    refused(a)                                                              # in the caller's units now
    for u, v in zip((a.X, a.y, a.S), tb[-3:]):
        assert same_bits(u, v)
    assert status_of(a) == status_of(b)
    # not initialised; more than one rank
    fresh = cuadmm_amd.SDPSolver(verbose=False)
    assert raw(fresh, Lv, Dv, ranks, RMAX, y, 0.7, 1.0)[0] == -1
    w = cuadmm_amd.SDPSolver(verbose=False, rank=0, world=2)
    w.set_allreduce(lambda ptr, count, stream: None)
    w.init_problem(amd(fx))
    assert raw(w, Lv, Dv, ranks, RMAX, y, 0.7, 1.0)[0] == -1 and b"one rank" in lib.cuadmm_last_error()
    # the Python front end
    bad = [m.copy() for m in Ds]
    bad[1] = np.zeros((20, 2))
    for args in ((Ls, bad, None, 0.5, 1.0), (Ls, Ds[:4], None, 0.5, 1.0), (Ls, Ds, y[:-1], 0.5, 1.0), (Ls, Ds, y, -1.0, 1.0), (Ls, Ds, y, 0.5, np.nan)):
        with pytest.raises(ValueError, match="lowrank_line"):
            a.lowrank_line(*args)
    # behind a failed cuadmm_update_A: CUADMM_ERR_FACTOR
    a.set_option("update_A_inject_fail", 1)                              # the test hook of tests/test_gpu_update_a.py
    with pytest.raises(cuadmm_amd.CuadmmError) as e:
        a.update_A(amd(fx).At_csc_vals * 1.5)
    assert e.value.code == -4
    rc, c, r, p, q, o, pb = raw(a, Lv, Dv, ranks, RMAX, y, 0.7, 1.0)
    assert rc == -4 and np.all(np.isnan(o)) and np.all(np.isnan(c)) and b"cuadmm_update_A" in lib.cuadmm_last_error()


def test_lowrank_descent():
    """five steps: each step's predicted f(t*) is the next step's f within the two bounds (the quartic's at t*, lowrank_grad's at the new
    factors; L + t* D is rounded there, two u on a factor relative to |L| + t* |D|, which the quartic's chain at t* is built on and whose
    K in the tens of thousands covers), the trace does not increase beyond them, and the last f is strictly below the first.  No rate is
    asserted."""
    fx, s, X0, y, sigma = start()
    Ls = factors(81)
    out = s.lowrank_descent(Ls, y, sigma=sigma, steps=5)
    tr = out["trace"]
    assert len(tr) == 5 and tr[0]["restart"] and all(t["t"] > 0 for t in tr)
    assert [m.shape for m in out["L"]] == [m.shape for m in Ls]
    K, Kg = constants(fx, RANKS), grad_constants(fx, RANKS)
    # replay on the host: the driver's own recurrence gives the factors and directions of every step
    inner_ = lambda A, B: float(sum(np.sum(a * b) for a, b in zip(A, B)))
    cur, D, G_old = [m.copy() for m in Ls], None, None
    for i, t in enumerate(tr):
        g = s.lowrank_grad(cur, y, sigma)
        assert same_bits(g["f"], t["f"]) and same_bits(g["gnorm"], t["gnorm"])
        G = g["G"]
        if D is None:
            D = [-a for a in G]
        else:
            beta = max(0.0, (inner_(G, G) - inner_(G, G_old)) / inner_(G_old, G_old))
            D = [-a + beta * d for a, d in zip(G, D)]
            if inner_(G, D) >= 0:
                D = [-a for a in G]
        tw = twin(fx, X0, cur, D, y, sigma)
        nxt = [a + t["t"] * d for a, d in zip(cur, D)]
        if i + 1 < len(tr):
            allow = coef_bound(tw, K, t["t"]) + gamma(Kg["f"] + 4) * grad_twin(fx, X0, nxt, y, sigma)["fb"]
            print("step %d: f %.12e, t %.3e, predicted %.12e, next f %.12e, allowance %.3e" % (i, t["f"], t["t"], t["predicted"], tr[i + 1]["f"], float(allow)))
            assert abs(LD(t["predicted"]) - LD(tr[i + 1]["f"])) <= allow
            assert LD(tr[i + 1]["f"]) <= LD(t["f"]) + allow
        cur, G_old = nxt, G
    assert tr[-1]["f"] < tr[0]["f"]
    assert all(same_bits(a, b) for a, b in zip(out["L"], cur))
    assert same_bits(s.X, X0)


# ---- 4. calls of different rmax on one solver -----------------------------------------------------------------------------
# 3: inside one tile; 20: two tiles and a rank above 16; -2: a free block that shifts every later offset; 33: above kLoWaveMax (the outer
# product's workgroup path, three panels of the block product).  (name, rmax, ranks, which): every ranks has a block at rank 0 and one at
# min(n, rmax).
BLK_I, M_I = [3, 20, -2, 33], 5
MIX = (("block_multiply", 4, (3, 0, 0, 4), 2), ("lowrank_grad", 20, (0, 20, 0, 7), 0), ("lowrank_line", 1, (1, 0, 0, 1), 0), ("set_lowrank", 33, (0, 17, 0, 33), 0),
       ("lowrank_grad", 4, (3, 4, 0, 0), 0), ("block_multiply", 33, (3, 0, 0, 33), 0), ("lowrank_line", 20, (0, 20, 0, 13), 0), ("lowrank", 4, None, 0))


def mix_call(s, fx, step):
    """every output of call `step` of MIX on s but the milliseconds and the bytes held, as a list of arrays"""
    name, rmax, ranks, which = MIX[step]
    lib = cuadmm_amd.load()
    rng = np.random.default_rng(900 + step)
    nb, size = len(BLK_I), max(lowrank_size(BLK_I, rmax), 1)
    y = rng.standard_normal(fx.m)
    o = np.full(8, np.nan)
    if name == "lowrank":
        pb, L, piv = np.full(6 * nb, np.nan), np.full(size, np.nan), np.full(size, -7, np.int32)
        assert lib.cuadmm_lowrank(s._h, which, 1e-8, rmax, P(o), P(pb), P(L), P(piv)) == 0, lib.cuadmm_last_error()
        return [o[:6], pb, L, piv.astype(np.float64)]
    Fs = [[rng.standard_normal((max(n, 0), r if n > 0 else 0)) for n, r in zip(BLK_I, ranks)] for _ in range(2)]
    (Lv, rk), (Dv, _) = pack(BLK_I, Fs[0], rmax), pack(BLK_I, Fs[1], rmax)      # NaN in every column that must not be read
    if name == "set_lowrank":
        o4 = np.full(4, np.nan)
        assert lib.cuadmm_set_lowrank(s._h, which, P(Lv), P(rk), rmax, 0.0, P(o4)) == 0, lib.cuadmm_last_error()
        assert o4[3] == 8 * lowrank_size(BLK_I, rmax)
        return [o4[[0, 1, 3]], s.X]
    if name == "block_multiply":
        W, pb = np.full(size, np.nan), np.full(4 * nb, np.nan)
        assert lib.cuadmm_block_multiply(s._h, which, P(Lv), P(rk), rmax, P(W), P(o), P(pb)) == 0, lib.cuadmm_last_error()
        return [o[:6], W, pb]
    if name == "lowrank_grad":
        G, r, Sh, pb = np.full(size, np.nan), np.full(fx.m, np.nan), np.full(fx.L, np.nan), np.full(4 * nb, np.nan)
        assert lib.cuadmm_lowrank_grad(s._h, P(Lv), P(rk), rmax, P(y), 0.7, P(G), P(r), P(Sh), P(o), P(pb)) == 0, lib.cuadmm_last_error()
        return [o[:6], G, r, Sh, pb]
    rc, c, r, p, q, o, pb = raw(s, Lv, Dv, rk, rmax, y, 0.7, 2.0, m=fx.m, nb=nb)
    assert rc == 0, lib.cuadmm_last_error()
    return [o[:6], c, r, p, q, pb]


@pytest.mark.parametrize("iters", [0, 10])
def test_calls_of_different_rmax_on_one_solver(iters):
    """The eight calls of MIX in turn on one solver, each with an rmax of its own: every output equals, bit for bit, that of the same call
    made alone on a fresh solver -- behind nothing for the calls before set_lowrank, behind that set_lowrank alone for the calls after
    it.  iters = 10: behind a solve, where X lies scaled and the factors are staged times fl(1 / sqrt(bscale)) (until set_lowrank puts
    the solver back into the caller's units)."""
    fx = make_opt_fixture(BLK_I, M_I, 3)
    X0 = np.random.default_rng(91).standard_normal(fx.L)
    SET = [c[0] for c in MIX].index("set_lowrank")

    def fresh():
        s = solver(fx, X0)
        if iters:
            s.solve(iters, 0.0)
        return s

    one = fresh()
    got = [mix_call(one, fx, step) for step in range(len(MIX))]
    assert all(np.isfinite(a).all() for step in (1, 2, 4, 6) for a in got[step])
    for step in range(len(MIX)):
        alone = fresh()
        if step > SET:
            mix_call(alone, fx, SET)
        want = mix_call(alone, fx, step)
        assert len(want) == len(got[step]) and all(same_bits(a, b) for a, b in zip(got[step], want)), (step, MIX[step][:2])


# ---- 5. the front ends ----------------------------------------------------------------------------------------------------
BLK_C, M_C = [3, 12, -2, 20], 10


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


def test_the_front_ends_return_the_same_bits(tmp_path):
    """The command line always solves first, so it is compared with the binding (which calls the C entry, compared with it bit for bit in
    test_against_the_twin_and_lowrank_grad) behind the same 40 iterations."""
    fx = make_opt_fixture(BLK_C, M_C, 5)
    d, ldir, ddir = str(tmp_path / "prob") + "/", str(tmp_path / "L") + "/", str(tmp_path / "D") + "/"
    _write_txt(d, fx)
    Ls = [np.array([[(i + 1) / (t + 2) - k for t in range(2)] for i in range(n)]) if n > 0 else np.zeros((0, 0)) for k, n in enumerate(BLK_C)]
    Ds = [np.array([[(t + 1) / (i + 2) - 0.25 * k for t in range(2)] for i in range(n)]) if n > 0 else np.zeros((0, 0)) for k, n in enumerate(BLK_C)]
    y1 = ((np.arange(M_C) * 5) % 9 - 4) / 8.0
    for dd, Fs in ((ldir, Ls), (ddir, Ds)):
        os.makedirs(dd)
        for k, n in enumerate(BLK_C):
            if n > 0:
                with open(dd + "L_X_%d.txt" % k, "w") as f:
                    f.write("".join("%.17g\n" % x for x in Fs[k].T.ravel()))
    exe = os.path.join(ROOT, "cuadmm_amd", "lib", "cuadmm_exe")
    for with_y, spec, t_max in ((False, "0.7", INF), (True, "0.7,2.5", 2.5)):
        if with_y:
            with open(ldir + "y.txt", "w") as f:
                f.write("".join("%.17g\n" % x for x in y1))
        s = cuadmm_amd.SDPSolver(verbose=False, profile=True)
        s.init_problem(cuadmm_amd.Problem.from_txt(d))
        s.solve(40, 0.0, 0, 50, 100, 5000, 1.05)
        py = s.lowrank_line(Ls, Ds, y1 if with_y else None, 0.7, t_max)
        js = str(tmp_path / ("ll%d.json" % with_y))
        r = subprocess.run([exe, d, "--lowrank-line=%s,%s,%s" % (ldir, ddir, spec), "--max_iter=40", "--stop_tol=0", "--quiet", "--json=" + js],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.count(" lowrank_line(sigma = 0.7") == 1
        with open(js) as f:
            side = json.load(f)["lowrank_line"]
        assert side["sigma"] == 0.7 and side["rmax"] == 2 and side["y"] is with_y
        assert same_bits(side["coef"], py["coef"]) and side["t"] == py["t"] and side["f"] == py["f"], with_y
    for args in (["--lowrank-line=" + ldir], ["--lowrank-line=%s,%s,-1" % (ldir, ddir)], ["--lowrank-line=%s,%s,0.7,x" % (ldir, ddir)],
                 ["--lowrank-line=%s,%snone/" % (ldir, ddir)]):
        r = subprocess.run([exe, d, "--quiet"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--lowrank-line" in r.stderr, args
