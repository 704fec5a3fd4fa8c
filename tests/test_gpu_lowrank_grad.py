"""Value and gradient at factors on the GPU (include/cuadmm_amd.h: cuadmm_lowrank_grad, cuadmm_op_lrg_multiplier; csrc/lowrank_grad.h;
DESIGN.md, "Value and gradient at factors"): the multiplier pass through its op hook, then the solver entry against the longdouble twin of
tests/_lowrank_grad_twin.py, its ties to cuadmm_block_multiply and cuadmm_evaluate, the five-point identity through the device, the solve
that continues bit for bit, the refusals and the three front ends.

Tolerances, none of them measured (u = 2^-53): every output within gamma(K) times its absolute-value chain, K counted from the code launch
by launch in the twin's docstring (constants()); what the host forms from the returned G is compared bit for bit.  On fixture A with ranks
(3, 20, 6, 0, 9): c = 11218 entries per row of A, c' = 40 per row of A', R = 20, n = 130, m = 40, vec_len = 11218, so
K_r = 11254, K_y = 11259, K_S = 11302, K_G = 11437, K_cx = 11254, K_yr = 11564, K_rr = 22814, K_f = 22816.
Measured share of the bound on the MI355X (largest err / bound over the entries): see NOTEBOOK.md, Round 20."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from tests._block_mult_twin import LD, loffs, lowrank_size, offsets, pack, seq_dot, unpack
from tests._lower_bound_twin import make_opt_fixture
from tests._lowrank_grad_twin import constants, five_point, gamma, inner, twin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
BLK_A, M_A = [3, 20, 70, -2, 130], 40          # the fixture of tests/test_gpu_block_mult.py
RANKS = (3, 20, 6, 0, 9)                       # rank 0 (the free block's is ignored), a rank above 16, full rank on the smallest block
RMAX = 20
INFO = ("pobj", "dobj", "errRp", "errRd", "relgap", "sig", "bscale", "Cscale")
_fx = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def share(err, bound):
    """largest err / bound over the entries, printed beside every check"""
    err, bound = np.atleast_1d(np.asarray(err, LD)), np.atleast_1d(np.asarray(bound, LD))
    return float(np.max(err / np.maximum(bound, np.finfo(LD).tiny))) if err.size else 0.0


# ---- 1. the multiplier pass -----------------------------------------------------------------------------------------------
def multiplier(ax, b, normA, y, bscale, Cscale, sigma):
    m = ax.size
    yt, r, o = np.full(m, np.nan), np.full(m, np.nan), np.full(2, np.nan)
    rc = cuadmm_amd.load().cuadmm_op_lrg_multiplier(m, P(ax), P(b), P(normA), P(y), bscale, Cscale, sigma, P(yt), P(r), P(o))
    assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
    assert not np.any(np.isnan(yt)) and not np.any(np.isnan(r)) and not np.any(np.isnan(o))
    return yt, r, o


@pytest.mark.parametrize("sigma", [0.0, 0.5, 3.7])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_multiplier_pass(m, sigma):
    """Roundings, from csrc/lowrank_grad.hip (lg_one): r takes 3 (the subtraction, the products by normA and bscale); the scaled sigma r
    r's 3, three products and fl(1 / Cscale), 7, and the subtraction from y 1: 8 on |y| + |sigma r| scaled; y'r: the subtraction, the
    product, a term's path through the sums (its thread's terms, the workgroup's tree, 256 slots: at most m + 264) and the unit's 2; ||r||^2:
    2 x 3 + 1 on a square and the same path."""
    rng = np.random.default_rng(1000 * m + int(10 * sigma))
    ax, b, y = (rng.standard_normal(m) * np.exp(rng.uniform(-2, 2, size=m)) for _ in range(3))
    normA = rng.uniform(1.0, 3.0, size=m)
    bscale, Cscale = 1 + 2.3 * rng.random(), 1 + 5.1 * rng.random()
    yt, r, o = multiplier(ax, b, normA, y, bscale, Cscale, sigma)
    l = lambda a: np.asarray(a).astype(LD)
    rs, rsb = l(ax) - l(b), np.abs(l(ax)) + np.abs(l(b))
    rx, rb = l(normA) * rs * LD(bscale), l(normA) * rsb * LD(bscale)
    assert np.all(np.abs(l(r) - rx) <= gamma(3) * rb)
    ytx, ytb = l(y) - LD(sigma) * rx * l(normA) / LD(Cscale), np.abs(l(y)) + LD(sigma) * rb * l(normA) / LD(Cscale)
    if sigma == 0.0:
        assert same_bits(yt, y)
    else:
        assert np.all(np.abs(l(yt) - ytx) <= gamma(8) * ytb)
    unit = LD(bscale) * LD(Cscale)
    assert abs(LD(o[0]) - np.sum(l(y) * rs) * unit) <= gamma(m + 268) * np.sum(np.abs(l(y)) * rsb) * unit
    assert abs(LD(o[1]) - np.sum(rx * rx)) <= gamma(m + 271) * np.sum(rb * rb)
    again = multiplier(ax, b, normA, y, bscale, Cscale, sigma)
    assert all(same_bits(u, v) for u, v in zip(again, (yt, r, o)))


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_multiplier_pass_is_exact_on_integers(m):
    """small integers, powers of two for normA, bscale and Cscale, sigma = 0.5: every product, difference and sum is exact"""
    rng = np.random.default_rng(m)
    ax, b, y = (rng.integers(-9, 10, size=m).astype(np.float64) for _ in range(3))
    normA = 2.0 ** rng.integers(0, 3, size=m)
    bscale, Cscale, sigma = 4.0, 2.0, 0.5
    yt, r, o = multiplier(ax, b, normA, y, bscale, Cscale, sigma)
    rs = ax - b
    want_r = normA * rs * bscale
    assert same_bits(r, want_r) and same_bits(yt, y - sigma * want_r * normA / Cscale)
    assert o[0] == float(np.sum(y * rs)) * bscale * Cscale and o[1] == float(np.sum(want_r * want_r))


# ---- 2. the solver entry --------------------------------------------------------------------------------------------------
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


def factors(seed, ranks=RANKS, dyadic=False):
    rng = np.random.default_rng(seed)
    if dyadic:                                                              # multiples of 2^-10 in [-2, 2]
        return [rng.integers(-2048, 2049, size=(max(n, 0), r if n > 0 else 0)) / 1024.0 for n, r in zip(BLK_A, ranks)]
    return [rng.standard_normal((max(n, 0), r if n > 0 else 0)) for n, r in zip(BLK_A, ranks)]


def raw(s, Lv, ranks, rmax, y, sigma, G=True, r=True, Sh=True, out=True, pb=True):
    """(rc, G buffer, r, Shat, out8, per_block) of cuadmm_lowrank_grad; the outputs pre-filled with NaN"""
    fx = fixture()
    Gb = np.full(max(lowrank_size(BLK_A, max(min(rmax, 8192), 1)), 1), np.nan) if G else None
    rv = np.full(fx.m, np.nan) if r else None
    Sv = np.full(fx.L, np.nan) if Sh else None
    o = np.full(8, np.nan) if out else None
    p = np.full(4 * len(BLK_A), np.nan) if pb else None
    rc = cuadmm_amd.load().cuadmm_lowrank_grad(s._h, P(Lv), P(ranks), rmax, P(y), float(sigma), P(Gb), P(rv), P(Sv), P(o), P(p))
    return rc, Gb, rv, Sv, o, p


def host_sums(Ls, Gs):
    """per_block[:, 1:4] of the PSD blocks and out8[4:6] as the call forms them from the returned G and the caller's L"""
    pb = np.zeros((len(BLK_A), 3))
    sq_all = dot_all = 0.0
    for k, n in enumerate(BLK_A):
        if n > 0:
            g, l = Gs[k].T.ravel(), np.asarray(Ls[k], np.float64).T.ravel()
            sq, dot, lsq = seq_dot(g, g), seq_dot(l, g), seq_dot(l, l)
            pb[k] = np.sqrt(sq), dot, lsq
            sq_all, dot_all = sq_all + sq, dot_all + dot
    return pb, np.array([np.sqrt(sq_all), dot_all])


def check_against_twin(tw, K, Ls, Gs, r, Sh, o, pb, what):
    """every output within gamma(K) of its chain; prints the measured share of each bound"""
    l = lambda a: np.asarray(a).astype(LD)
    off = offsets(BLK_A)
    sh = {}
    for k, n in enumerate(BLK_A):
        if n > 0 and Ls[k].shape[1] > 0:
            err, bound = np.abs(l(Gs[k]) - tw["G"][k]), gamma(K["G"]) * tw["Gb"][k]
            sh["G"] = max(sh.get("G", 0.0), share(err, bound))
            assert np.all(err <= bound), (what, "G", k)
    for name, got, ref, bound in (("r", r, tw["r"], gamma(K["r"]) * tw["rb"]), ("Shat", Sh, tw["Sh"], gamma(K["S"]) * tw["Sb"]),
                                  ("f", o[0], tw["f"], gamma(K["f"]) * tw["fb"]), ("cx", o[1], tw["cx"], gamma(K["cx"]) * tw["cxb"]),
                                  ("yr", o[2], tw["yr"], gamma(K["yr"]) * tw["yrb"]),
                                  ("rnorm", o[3], np.sqrt(tw["rr"]), gamma(K["rr"]) * np.sqrt(tw["rrb"]))):
        if got is None:
            continue
        err = np.abs(l(got) - ref)
        sh[name] = share(err, bound)
        assert np.all(err <= bound), (what, name, sh[name])
    nG = sum(g.size for g in Gs)
    absL = [np.abs(l(m)) for m in Ls]
    gn, gnb = np.sqrt(inner(tw["G"], tw["G"])), np.sqrt(inner(tw["Gb"], tw["Gb"]))
    assert abs(LD(o[4]) - gn) <= gamma(K["G"] + nG) * gnb, (what, "gnorm")
    assert abs(LD(o[5]) - inner(tw["G"], Ls)) <= gamma(K["G"] + nG + 1) * inner(tw["Gb"], absL), (what, "lg")
    C = np.abs(l(fixture().C))
    for k, n in enumerate(BLK_A):
        sl = slice(off[k], off[k + 1])
        cxk, cxkb = np.sum(l(fixture().C)[sl] * tw["x"][sl]), np.sum(C[sl] * tw["xb"][sl])
        assert abs(LD(pb[k, 0]) - cxk) <= gamma(K["cx"]) * cxkb, (what, "per_block 0", k)
        if n < 0:
            ref, bound = np.sqrt(np.sum(tw["Sh"][sl] ** 2)), gamma(K["S"] + (off[k + 1] - off[k])) * np.sqrt(np.sum(tw["Sb"][sl] ** 2))
            assert abs(LD(pb[k, 1]) - ref) <= bound and pb[k, 2] == 0 and pb[k, 3] == 0, (what, "per_block free", k)
            continue
        e = Gs[k].size
        Gk, Gkb, Lk = tw["G"][k], tw["Gb"][k], l(Ls[k])
        assert abs(LD(pb[k, 1]) - np.sqrt(np.sum(Gk * Gk))) <= gamma(K["G"] + e) * np.sqrt(np.sum(Gkb * Gkb)), (what, "per_block 1", k)
        assert abs(LD(pb[k, 2]) - np.sum(Lk * Gk)) <= gamma(K["G"] + e + 1) * np.sum(np.abs(Lk) * Gkb), (what, "per_block 2", k)
        assert abs(LD(pb[k, 3]) - np.sum(Lk * Lk)) <= gamma(e + 1) * np.sum(Lk * Lk), (what, "per_block 3", k)
    print(what, "share of the bound:", ", ".join("%s %.2e" % kv for kv in sorted(sh.items())))
    return sh


def start():
    """(fixture, solver, X, y, sigma): a fresh solver given a random X0, so that the free slice of x matters; X: what the solver holds
    after init (its getter; the caller's units, nothing pending), which is what the twin is evaluated at"""
    fx = fixture()
    rng = np.random.default_rng(41)
    s = solver(fx, rng.standard_normal(fx.L))
    X = s.X
    off = offsets(BLK_A)
    assert np.all(X[off[3]:off[4]] != 0)
    return fx, s, X, rng.standard_normal(fx.m), 0.7


def test_against_the_twin():
    fx, s, X0, y, sigma = start()
    Ls = factors(43)
    Lv, ranks = pack(BLK_A, Ls, RMAX)                                       # NaN in every column that must not be read
    assert np.isnan(Lv).any()
    rc, Gb, r, Sh, o, pb = raw(s, Lv, ranks, RMAX, y, sigma)
    assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
    assert not np.isnan(Gb[:lowrank_size(BLK_A, RMAX)]).any() and not any(np.isnan(v).any() for v in (r, Sh, o, pb))
    Gs, pads = unpack(BLK_A, ranks, RMAX, Gb)
    assert all(same_bits(p, np.zeros(p.size)) for p in pads)                # columns >= r_k of G are + 0.0
    pb = pb.reshape(-1, 4)
    check_against_twin(twin(fx, X0, Ls, y, sigma), constants(fx, RANKS), Ls, Gs, r, Sh, o, pb, "fresh solver:")
    tpb, to = host_sums(Ls, Gs)
    psd = [k for k, n in enumerate(BLK_A) if n > 0]
    assert same_bits(pb[psd, 1:], tpb[psd]) and same_bits(o[4:6], to)
    assert o[6] > 0 and o[7] >= 8 * (fx.L + 4 * fx.m + 2 * lowrank_size(BLK_A, RMAX))
    assert same_bits(o[1], np.cumsum(pb[:, 0])[-1])                         # <C, x>: the blocks' terms added in block order
    # the outputs that may be null; the same bits from run to run and through the Python front end
    rc2, G2, _, _, o2, _ = raw(s, Lv, ranks, RMAX, y, sigma, r=False, Sh=False, pb=False)
    assert rc2 == 0 and same_bits(G2, Gb) and same_bits(o2[:6], o[:6])
    rc3, _, r3, _, o3, _ = raw(s, Lv, ranks, RMAX, y, sigma, G=False, Sh=False)
    assert rc3 == 0 and same_bits(r3, r) and same_bits(o3[:6], o[:6])
    py = s.lowrank_grad(Ls, y, sigma, want_S=True)
    assert all(same_bits(a, b) for a, b in zip(py["G"], Gs)) and same_bits(py["r"], r) and same_bits(py["Shat"], Sh) and same_bits(py["per_block"], pb)
    assert same_bits([py[k] for k in ("f", "cx", "yr", "rnorm", "gnorm", "lg")], o[:6]) and "Shat" not in s.lowrank_grad(Ls, y, sigma)
    assert same_bits(s.X, X0)                                               # the resident X keeps its bits


def test_sigma_zero_is_twice_the_dual_product():
    fx, s, X0, y, _ = start()
    s.set_XyS(y=y)
    Ls = factors(47)
    W = s.block_multiply("dual", Ls)["W"]
    for arg in (None, y):
        g = s.lowrank_grad(Ls, arg, 0.0)
        assert all(same_bits(a, 2 * b) for a, b in zip(g["G"], W))
    assert g["yr"] != 0 and same_bits(g["f"], g["cx"] - g["yr"])


def test_five_point_identity_through_the_device():
    """L, D multiples of 2^-10 in [-2, 2] and h = 2^-3: every L + t D is exact, t -> f(L + t D) is a quartic, and the five-point formula is
    <G(L), D> exactly.  f is within gamma(K_f) fbar at each point (weights 1 + 8 + 8 + 1 over 12 h), <G, D> within gamma(K_G) <Gbar, |D|>."""
    fx, s, X0, y, sigma = start()
    Ls, Ds = factors(53, dyadic=True), factors(59, dyadic=True)
    h = 2.0 ** -3
    K = constants(fx, RANKS)
    fs, fbs = [], []
    for t in (-2 * h, -h, h, 2 * h):
        Lt = [L + t * D for L, D in zip(Ls, Ds)]
        assert all(np.array_equal((a - b) / t, d) for a, b, d in zip(Lt, Ls, Ds))
        fs.append(s.lowrank_grad(Lt, y, sigma)["f"])
        fbs.append(twin(fx, X0, Lt, y, sigma)["fb"])
    G = s.lowrank_grad(Ls, y, sigma)["G"]
    lhs, rhs = five_point(fs, h), inner(G, Ds)
    tol = 18 / (12 * LD(h)) * gamma(K["f"]) * max(fbs) + gamma(K["G"]) * inner(twin(fx, X0, Ls, y, sigma)["Gb"], [np.abs(D) for D in Ds])
    print("five-point %.15Lg, <G, D> %.15Lg, difference %.3Lg, tolerance %.3Lg" % (lhs, rhs, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol and abs(rhs) > 100 * tol


def _traj(s):
    return [s.info_arr(k).copy() for k in INFO] + [s.X, s.y, s.S]


def test_behind_a_solve():
    """a: 30 iterations, the call on the pending scaled state, 30 more; b: the same without the call; c: 30 iterations, the call, the
    getters; d: 30 iterations and the getters, which the twin is evaluated at (the getters' unscaling: one rounding on X, three on y,
    inside what K_r and K_y allow the staged vectors)."""
    fx = fixture()
    a, b, c, d = (solver(fx) for _ in range(4))
    for s in (a, b, c, d):
        s.solve(30, 0.0)
    Ls = factors(61)
    sigma = 0.7
    ga, gc = a.lowrank_grad(Ls, None, sigma, want_S=True), c.lowrank_grad(Ls, None, sigma, want_S=True)
    assert all(same_bits(u, v) for u, v in zip(ga["G"], gc["G"])) and same_bits(ga["f"], gc["f"])
    o = np.array([gc[k] for k in ("f", "cx", "yr", "rnorm", "gnorm", "lg")])
    check_against_twin(twin(fx, d.X, Ls, d.y, sigma), constants(fx, RANKS), Ls, gc["G"], gc["r"], gc["Shat"], o, gc["per_block"], "behind a solve:")
    for u, v in zip((c.X, c.y, c.S), (d.X, d.y, d.S)):
        assert same_bits(u, v)
    for s in (a, b):
        s.solve(30, 0.0, if_first=False)
    for u, v in zip(_traj(a), _traj(b)):
        assert same_bits(u, v)
    assert a.info_iter_num == b.info_iter_num == 30


def test_r_against_evaluate():
    """||A x - b|| of evaluate() on a second solver whose X was set from the same factors agrees with rnorm within the twin's allowance
    for r, and each lies within it of the twin"""
    fx, s, X0, y, sigma = start()
    t = start()[1]
    Ls = factors(67)
    g = s.lowrank_grad(Ls, y, sigma)
    t.set_lowrank(X=Ls)
    ev = t.evaluate()
    tw = twin(fx, X0, Ls, y, sigma)
    allow = gamma(constants(fx, RANKS)["rr"]) * np.sqrt(tw["rrb"])
    print("rnorm %.15e, evaluate %.15e, difference %.3e, allowance %.3e" % (g["rnorm"], ev["norm_Rp"], abs(g["rnorm"] - ev["norm_Rp"]), float(allow)))
    assert abs(LD(g["rnorm"]) - LD(ev["norm_Rp"])) <= allow
    assert abs(LD(g["rnorm"]) - np.sqrt(tw["rr"])) <= allow and abs(LD(ev["norm_Rp"]) - np.sqrt(tw["rr"])) <= allow


def status_of(s):
    st = s.status()
    return {k: st[k] for k in st if k not in ("ms", "check_ms")}


def test_refusals_leave_the_solver_as_it_was():
    fx = fixture()
    lib = cuadmm_amd.load()
    a, b = solver(fx), solver(fx)
    for s in (a, b):
        s.solve(20, 0.0)
    Ls = factors(71)
    Lv, ranks = pack(BLK_A, Ls, RMAX)
    y = np.random.default_rng(73).standard_normal(fx.m)
    lo = loffs(BLK_A, RMAX)

    def with_rank(k, r):
        q = ranks.copy()
        q[k] = r
        return q

    def with_entry(k, col, row, x):
        q = Lv.copy()
        q[lo[k] + col * BLK_A[k] + row] = x
        return q

    def refused(s):
        for L_, ranks_, rmax_, y_, sigma_ in ((Lv, ranks, RMAX, y, -0.5), (Lv, ranks, RMAX, y, np.nan), (Lv, ranks, RMAX, None, np.inf), (Lv, ranks, 0, y, 0.7),
                                              (Lv, ranks, 8193, y, 0.7), (Lv, None, RMAX, y, 0.7), (Lv, with_rank(1, -1), RMAX, y, 0.7),
                                              (Lv, with_rank(2, 21), RMAX, y, 0.7), (Lv, with_rank(0, 4), RMAX, y, 0.7), (None, ranks, RMAX, y, 0.7),
                                              (with_entry(2, 5, 69, np.nan), ranks, RMAX, y, 0.7), (with_entry(4, 0, 0, np.inf), ranks, RMAX, None, 0.7),
                                              (Lv, ranks, RMAX, np.where(np.arange(fx.m) == 7, np.nan, y), 0.7)):
            rc, G, r, Sh, o, pb = raw(s, L_, ranks_, rmax_, y_, sigma_)
            assert rc == -1 and all(np.all(np.isnan(v)) for v in (G, r, Sh, o, pb)), (rmax_, sigma_)      # CUADMM_ERR_INVALID, outputs untouched
            assert "lowrank_grad" in lib.cuadmm_last_error().decode()
        assert raw(s, Lv, ranks, RMAX, y, 0.7, out=False)[0] == -1
    assert np.isnan(Lv[lo[2] + 6 * 70])                                     # a NaN in a column that is not read is no reason to refuse
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
    # not initialised; more than one rank; the leader of an in-process group
    fresh = cuadmm_amd.SDPSolver(verbose=False)
    assert raw(fresh, Lv, ranks, RMAX, y, 0.7)[0] == -1
    w = cuadmm_amd.SDPSolver(verbose=False, rank=0, world=2)
    w.set_allreduce(lambda ptr, count, stream: None)
    w.init_problem(amd(fx))
    assert raw(w, Lv, ranks, RMAX, y, 0.7)[0] == -1 and "one rank" in lib.cuadmm_last_error().decode()
    blk_g = [6, 10, 6, 10]                                                  # (the duo front end takes two block sizes)
    p = amd(make_opt_fixture(blk_g, 8, 9))
    g = cuadmm_amd.SDPSolver(verbose=False, options={"duo_share_device": 1})
    g.duo_init(True, 2, 15, 30, p.vec_len, p.con_num, p.At_csc_col_ptrs, p.At_csc_row_ids, p.At_csc_vals, p.At_nnz, p.b_indices, p.b_vals, p.b_nnz,
               p.C_indices, p.C_vals, p.C_nnz, p.blk_vals, p.mat_num)
    assert g.group_info()["engines"] == 2
    Lg, rg = pack(blk_g, [np.ones((n, 2)) for n in blk_g], 2)
    Xg = g.X
    o = np.full(8, np.nan)
    assert lib.cuadmm_lowrank_grad(g._h, P(Lg), P(rg), 2, None, 0.0, P(np.zeros(Lg.size)), None, None, P(o), None) == -1
    assert "one rank" in lib.cuadmm_last_error().decode() and np.all(np.isnan(o)) and same_bits(g.X, Xg)
    # the Python front end
    bad = [m.copy() for m in Ls]
    bad[1] = np.zeros((19, 2))
    for args in ((bad, None, 0.0), (Ls[:4], None, 0.0), (Ls, y[:-1], 0.0), (Ls, y, -1.0), (Ls, y, np.nan)):
        with pytest.raises(ValueError, match="lowrank_grad"):
            a.lowrank_grad(*args)
    # behind a failed cuadmm_update_A: CUADMM_ERR_FACTOR
    a.set_option("update_A_inject_fail", 1)                              # the test hook of tests/test_gpu_update_a.py
    with pytest.raises(cuadmm_amd.CuadmmError) as e:
        a.update_A(amd(fx).At_csc_vals * 1.5)
    assert e.value.code == -4
    rc, G, r, Sh, o, pb = raw(a, Lv, ranks, RMAX, y, 0.7)
    assert rc == -4 and np.all(np.isnan(o)) and np.all(np.isnan(G)) and "cuadmm_update_A" in lib.cuadmm_last_error().decode()


# ---- 3. the front ends ----------------------------------------------------------------------------------------------------
FACADE = r'''
#include <cstdio>
#include <cstring>
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
    // the point of start_point() in the test: no solve, so that the state is the same in every front end by construction
    std::vector<double> X0((size_t)problem.vec_len), S0((size_t)problem.vec_len), y0((size_t)problem.con_num), y1((size_t)problem.con_num);
    for (int i = 0; i < problem.vec_len; ++i) { X0[i] = (double)((i * 7) % 11 - 5) / 4.0; S0[i] = (double)((i * 5) % 13 - 6) / 8.0; }
    for (int j = 0; j < problem.con_num; ++j) { y0[j] = (double)((j * 3) % 7 - 3) / 2.0; y1[j] = (double)((j * 5) % 9 - 4) / 8.0; }
    SDPSolver solver;
    solver.set_option("verbose", 0.0);
    solver.init(15, 30, problem.vec_len, problem.con_num, problem.At_csc_col_ptrs.data(), problem.At_csc_row_ids.data(), problem.At_csc_vals.data(),
                problem.At_nnz, problem.b_indices.data(), problem.b_vals.data(), problem.b_nnz, problem.C_indices.data(), problem.C_vals.data(),
                problem.C_nnz, blk_vals.data(), problem.mat_num, X0.data(), y0.data(), S0.data(), 1.0);
    // L: two columns per PSD block, entry (row i, column t) of block k = (i + 1) / (t + 2) - k
    const int rmax = 2;
    std::vector<int> ranks;
    std::vector<double> L;
    for (size_t k = 0; k < blk_vals.size(); ++k) {
      const int n = blk_vals[k];
      ranks.push_back(n > 0 ? 2 : 0);
      for (int t = 0; n > 0 && t < 2; ++t)
        for (int i = 0; i < n; ++i) L.push_back((double)(i + 1) / (double)(t + 2) - (double)k);
    }
    for (int pass = 0; pass < 2; ++pass) {
      const SDPSolver::LowRankGrad g = solver.lowrank_grad(L.data(), ranks.data(), rmax, pass ? y1.data() : nullptr, 0.7, pass == 1);
      const double sc[6] = {g.f, g.cx, g.yr, g.rnorm, g.gnorm, g.lg};
      unsigned long long b0;
      std::printf("LG %d %zu %zu %zu", pass, g.G.size(), g.r.size(), g.Shat.size());
      for (double w : sc) { std::memcpy(&b0, &w, 8); std::printf(" %llx", b0); }
      for (double w : g.G) { std::memcpy(&b0, &w, 8); std::printf(" %llx", b0); }
      for (double w : g.r) { std::memcpy(&b0, &w, 8); std::printf(" %llx", b0); }
      std::printf("\n");
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cuadmm_amd: %s\n", e.what());
    return 3;
  }
  return 0;
}
'''
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


def start_point(vec_len, con_num):
    i, j = np.arange(vec_len), np.arange(con_num)
    return ((i * 7) % 11 - 5) / 4.0, ((j * 3) % 7 - 3) / 2.0, ((i * 5) % 13 - 6) / 8.0


def test_the_three_front_ends_return_the_same_bits(tmp_path):
    """The command line always solves first, so it is compared with the binding behind the same 40 iterations.  The C++ facade is compared
    with the binding at a point given to init (start_point): SDPSolver::solve of include/cuadmm_amd.hpp ends with fetch(), which runs the
    deferred unscaling, while the binding's solve leaves the scaled state pending (NOTEBOOK.md, Round 19) -- the same value and gradient
    to the rounding contract, but not the same bits.  At a point given to init both hold the same vectors."""
    fx = make_opt_fixture(BLK_C, M_C, 5)
    d, fdir, out = str(tmp_path / "prob") + "/", str(tmp_path / "factors") + "/", str(tmp_path / "g") + "/"
    _write_txt(d, fx)
    os.makedirs(fdir)
    os.makedirs(out)
    Ls = [np.array([[(i + 1) / (t + 2) - k for t in range(2)] for i in range(n)]) if n > 0 else np.zeros((0, 0)) for k, n in enumerate(BLK_C)]
    y1 = ((np.arange(M_C) * 5) % 9 - 4) / 8.0
    for k, n in enumerate(BLK_C):
        if n > 0:
            with open(fdir + "L_X_%d.txt" % k, "w") as f:
                f.write("".join("%.17g\n" % x for x in Ls[k].T.ravel()))
    libdir = os.path.join(ROOT, "cuadmm_amd", "lib")
    exe = os.path.join(libdir, "cuadmm_exe")
    solve_args = (40, 0.0, 0, 50, 100, 5000, 1.05)
    for with_y in (False, True):
        if with_y:
            with open(fdir + "y.txt", "w") as f:
                f.write("".join("%.17g\n" % x for x in y1))
        s = cuadmm_amd.SDPSolver(verbose=False, profile=True)
        s.init_problem(cuadmm_amd.Problem.from_txt(d))
        s.solve(*solve_args)
        py = s.lowrank_grad(Ls, y1 if with_y else None, 0.7)
        js = str(tmp_path / ("lg%d.json" % with_y))
        r = subprocess.run([exe, d, "--lowrank-grad=%s,0.7" % fdir, "--lowrank-grad-out=" + out, "--max_iter=40", "--stop_tol=0", "--quiet", "--json=" + js],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.count(" lowrank_grad(sigma = 0.7): ") == 1
        with open(js) as f:
            side = json.load(f)["lowrank_grad"]
        assert side["sigma"] == 0.7 and side["rmax"] == 2 and side["y"] is with_y
        for key in ("f", "cx", "yr", "rnorm", "gnorm", "lg"):
            assert side[key] == py[key], (with_y, key)
        files = [np.array(open(out + "G_%d.txt" % k).read().split(), np.float64).reshape(2, n).T if n > 0 else np.zeros((0, 0)) for k, n in enumerate(BLK_C)]
        assert all(same_bits(a, b) for a, b in zip(files, py["G"])), with_y
        assert same_bits(np.array(open(out + "r.txt").read().split(), np.float64), py["r"])
    # a directory without factor files, a bad sigma, the output directory without the call: exit code 1 before any device work
    for args in (["--lowrank-grad=" + out + "none/"], ["--lowrank-grad=%s,-1" % fdir], ["--lowrank-grad=%s,x" % fdir], ["--lowrank-grad-out=" + out]):
        r = subprocess.run([exe, d, "--quiet"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--lowrank-grad" in r.stderr, args
    # the C++ facade
    src, fexe = tmp_path / "facade.cpp", tmp_path / "facade"
    src.write_text(FACADE)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(fexe), "-L" + libdir,
                           "-lcuadmm_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"], timeout=300)
    r = subprocess.run([str(fexe), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("LG ")]
    assert len(lines) == 2
    prob = cuadmm_amd.Problem.from_txt(d)
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(prob, *start_point(prob.vec_len, prob.con_num))
    nG = lowrank_size(BLK_C, 2)
    for ln in lines:
        p = int(ln[1])
        py = s.lowrank_grad(Ls, y1 if p else None, 0.7, want_S=bool(p))
        assert [int(x) for x in ln[2:5]] == [nG, M_C, prob.vec_len if p else 0]
        want = np.concatenate([[py[k] for k in ("f", "cx", "yr", "rnorm", "gnorm", "lg")], np.concatenate([m.T.ravel() for m in py["G"]]), py["r"]])
        assert [int(x, 16) for x in ln[5:]] == [int(b) for b in bits(want)], p
