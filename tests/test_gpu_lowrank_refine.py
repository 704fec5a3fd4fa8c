"""Conjugate gradients over the factors on the GPU (include/cuadmm_amd.h: cuadmm_lowrank_refine, cuadmm_op_lrr_dots, cuadmm_op_lrr_direction,
cuadmm_op_lrr_step; csrc/lowrank_refine.h; DESIGN.md, "Refinement over factors"): the three new kernels through their op hooks, then the
solver entry replayed step by step with cuadmm_lowrank_grad, cuadmm_cg_update and cuadmm_lowrank_line on the host's copy of the factors,
its reasons to stop, the solve that continues bit for bit, the refusals and the front ends.

Tolerances, none of them measured (u = 2^-53).  The vectors the kernels write and everything the replay compares are bit for bit.  The
three sums: (count / 256 + 264) u sum |terms| of a longdouble sum, the slot-sum bound of test_quartic_sums (tests/test_gpu_lowrank_line.py).
A step's f(t) against the next step's c0: the allowance of test_lowrank_descent there (the quartic's bound at t plus lowrank_grad's at
the new factors, from the twins' counted constants)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from tests._block_mult_twin import LD, loffs, lowrank_size, pack, unpack
from tests._lower_bound_twin import make_opt_fixture
from tests._lowrank_grad_twin import constants as grad_constants, gamma, twin as grad_twin
from tests._lowrank_line_twin import U, constants, horner_bar, twin
from tests._lowrank_refine_twin import COUNTS, TRACE, cg_update, direction, dots_bound, dots_ref, grad, step, view

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
BLK_A, M_A = [3, 20, 70, -2, 130], 40          # fixture A of the low-rank tests
RANKS = (3, 20, 6, 0, 9)
RMAX = 20
INFO = ("pobj", "dobj", "errRp", "errRd", "relgap", "sig", "bscale", "Cscale")
INF = float("inf")
SENT = -7.25
_fx = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- 1. the three kernels -------------------------------------------------------------------------------------------------
def vectors(n, seed, integers=False):
    rng = np.random.default_rng(seed)
    if integers:
        return [rng.integers(-9, 10, size=n).astype(np.float64) for _ in range(3)]
    out = [rng.standard_normal(n) * np.exp(rng.uniform(-2, 2, size=n)) for _ in range(3)]
    for v in out:                                # signed zeros among the entries
        v[rng.random(n) < 0.1] = 0.0
        v[rng.random(n) < 0.1] = -0.0
    return out


def op_direction(W, unit, beta, restart, root, D, shift):
    n = W.size
    w, d = view(W, shift), view(D, shift, SENT)
    ds, go = view(np.full(n, np.nan), shift, SENT), view(np.full(n, np.nan), shift, SENT)
    rc = cuadmm_amd.load().cuadmm_op_lrr_direction(n, P(w), unit, beta, int(restart), root, P(d), P(ds), P(go))
    assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
    assert all(same_bits(v[n], SENT) for v in (d, ds, go))                   # the guards behind the end
    return d[:n].copy(), ds[:n].copy(), go[:n].copy()


def op_step(L, D, t, root, shift):
    n = L.size
    d, l, ls = view(D, shift), view(L, shift, SENT), view(np.full(n, np.nan), shift, SENT)
    rc = cuadmm_amd.load().cuadmm_op_lrr_step(n, t, root, P(d), P(l), P(ls))
    assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
    assert same_bits(l[n], SENT) and same_bits(ls[n], SENT)
    return l[:n].copy(), ls[:n].copy()


def op_dots(W, unit, G_old, D_old, shift):
    o = np.full(3, np.nan)
    rc = cuadmm_amd.load().cuadmm_op_lrr_dots(W.size, P(view(W, shift)), unit, P(view(G_old, shift)), P(view(D_old, shift)), P(o))
    assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
    return o


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", COUNTS)
def test_direction_and_step(n, shift):
    W, D, L = vectors(n, 10 * n + shift)
    unit, root = 1.7320508075688772, 0.6324555320336759
    G = grad(W, unit)
    for beta, restart in ((0.37, False), (0.0, False), (0.0, True), (2.5, True)):
        Din = np.full(n, np.nan) if restart else D                           # a restart does not read D
        d, ds, go = op_direction(W, unit, beta, restart, root, Din, shift)
        wd, wds = direction(G, D, beta, restart, root)
        assert same_bits(d, wd) and same_bits(ds, wds) and same_bits(go, G), (beta, restart)
    assert same_bits(op_direction(W, 1.0, 0.37, False, 1.0, D, shift)[1], -2.0 * W + 0.37 * D)      # unit = root = 1: both products exact
    for t in (0.8125, 3.3e-7, 0.0):
        l, ls = op_step(L, D, t, root, shift)
        wl, wls = step(L, D, t, root)
        assert same_bits(l, wl) and same_bits(ls, wls), t
    # t = 0 leaves L's bits (a - 0.0 of L may meet + 0.0 t D and become + 0.0, as in numpy: none here)
    Lp = np.where(L == 0, 0.0, L)
    assert same_bits(op_step(Lp, np.abs(D), 0.0, root, shift)[0], Lp)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", COUNTS)
def test_three_sums(n, shift):
    W, Go, Do = vectors(n, 20 * n + shift)
    unit = 1.7320508075688772
    o = op_dots(W, unit, Go, Do, shift)
    G = grad(W, unit)
    for j, (ref, bar) in enumerate(dots_ref(G, Go, Do)):
        err, bound = abs(LD(o[j]) - ref), dots_bound(n, bar)
        assert err <= bound, (j, float(err), float(bound))
    assert same_bits(op_dots(W, unit, Go, Do, shift), o)                     # the same bits on a second run
    # exact on small integers (unit = 0.5: G = W)
    W, Go, Do = vectors(n, n, True)
    o = op_dots(W, 0.5, Go, Do, shift)
    assert np.array_equal(o, np.array([np.sum(W * W), np.sum(W * Go), np.sum(W * Do)]))


def test_hooks_refuse():
    lib = cuadmm_amd.load()
    a, o = np.zeros(4), np.zeros(3)
    assert lib.cuadmm_op_lrr_dots(0, P(a), 1.0, P(a), P(a), P(o)) == -1 and lib.cuadmm_op_lrr_dots(3, None, 1.0, P(a), P(a), P(o)) == -1
    assert lib.cuadmm_op_lrr_direction(3, P(a), 1.0, 0.0, 0, 1.0, None, P(a), P(a)) == -1
    assert lib.cuadmm_op_lrr_step(3, 1.0, 1.0, P(a), None, P(a)) == -1


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


def factors(seed, ranks=RANKS, blk=BLK_A, scale=1.0):
    rng = np.random.default_rng(seed)
    return [scale * rng.standard_normal((max(n, 0), r if n > 0 else 0)) for n, r in zip(blk, ranks)]


def raw(s, Lv, ranks, rmax, y, sigma, steps, t_max, gtol, m=M_A, alias=False, want=(True, True, True)):
    """(rc, L_out, trace (steps, 16), out8, r) of cuadmm_lowrank_refine; the outputs pre-filled with NaN"""
    size = Lv.size if Lv is not None else 1
    Lo = Lv if alias else (np.full(size, np.nan) if want[0] else None)
    tr = np.full(16 * max(steps, 1), np.nan) if want[1] else None
    o = np.full(8, np.nan) if want[2] else None
    r = np.full(m, np.nan)
    rc = cuadmm_amd.load().cuadmm_lowrank_refine(s._h, P(Lv), P(ranks), rmax, P(y), float(sigma), int(steps), float(t_max), float(gtol), P(Lo), P(tr), P(o), P(r))
    return rc, Lo, None if tr is None else tr.reshape(-1, 16), o, r


def flat(blk, Fs, rmax):
    return pack(blk, Fs, rmax, 0.0)[0]


def coef_bound(tw, K, t):
    return sum(gamma(K["c%d" % j]) * tw["cb"][j] * abs(LD(t)) ** j for j in range(5)) + 8 * LD(U) * horner_bar(tw["cb"], t)


def replay(s, fx, X0, y_twin, y_call, Ls, sigma, steps, blk=BLK_A, ranks=RANKS, rmax=RMAX, allowances=True):
    """cuadmm_lowrank_refine on s from Ls with NaN in every column that must not be read, then every step again on the host's copy of the
    factors with lowrank_grad, cg_update and lowrank_line.  y_call: what the calls are given (None: the resident y); y_twin: its value."""
    Lv, rk = pack(blk, Ls, rmax)
    assert np.isnan(Lv).any()
    rc, Lo, tr, o, r = raw(s, Lv, rk, rmax, y_call, sigma, steps, INF, 0.0, m=fx.m)
    assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
    assert o[0] == steps and o[1] == 0 and not np.isnan(tr).any() and not np.isnan(Lo).any() and np.all(tr[:, 14:] == 0) and np.all(tr[:, 13] > 0)
    count = lowrank_size(blk, rmax)
    if allowances:
        K, Kg = constants(fx, ranks), grad_constants(fx, ranks)
    cur, D, D_flat, G_old = [m.copy() for m in Ls], None, np.zeros(count), np.zeros(count)
    gg_prev = 0.0
    for k in range(steps):
        row = dict(zip(TRACE, tr[k]))
        g = s.lowrank_grad(cur, y_call, sigma)
        G = flat(blk, g["G"], rmax)
        for j, (ref, bar) in enumerate(dots_ref(G, G_old, D_flat)):
            assert abs(LD(tr[k, j]) - ref) <= dots_bound(count, bar), (k, j)
        beta, slope, restart = cg_update(row["gg"], row["go"], row["gd"], gg_prev, k == 0)
        assert same_bits([row["beta"], row["slope"], row["restart"]], [beta, slope, float(restart)]), k
        D = [-a for a in g["G"]] if restart else [-a + beta * d for a, d in zip(g["G"], D)]
        ln = s.lowrank_line(cur, D, y_call, sigma, INF)
        assert same_bits(ln["coef"], tr[k, 6:11]) and same_bits([ln["t"], ln["f"]], tr[k, 11:13]), k
        if k == steps - 1:
            assert same_bits(r, ln["r"])                                    # r_out: the line search's r0 of the last step
        nxt = [a + ln["t"] * d for a, d in zip(cur, D)]
        if allowances and k + 1 < steps:
            tw = twin(fx, X0, cur, D, y_twin, sigma)
            allow = coef_bound(tw, K, ln["t"]) + gamma(Kg["f"] + 4) * grad_twin(fx, X0, nxt, y_twin, sigma)["fb"]
            print("step %d: c0 %.12e, t %.3e, f(t) %.12e, next c0 %.12e, allowance %.3e" % (k, row["c0"], row["t"], row["f"], tr[k + 1, 6], float(allow)))
            assert abs(LD(row["f"]) - LD(tr[k + 1, 6])) <= allow
        cur, G_old, D_flat, gg_prev = nxt, G, flat(blk, D, rmax), row["gg"]
    Wo, pads = unpack(blk, rk, rmax, Lo)
    assert all(same_bits(a, b) for a, b in zip(Wo, cur))
    assert all(same_bits(p, np.zeros(p.size)) for p in pads)                # + 0.0 in the columns >= r_k
    assert tr[0, 5] == 1 and tr[-1, 12] < tr[0, 6]
    assert same_bits(o[2:5], [tr[0, 6], tr[-1, 12], np.sqrt(tr[-1, 0])]) and o[5] > 0 and o[6] >= 8 * 4 * count and o[7] == 0
    return tr, Wo


def start():
    fx = fixture()
    rng = np.random.default_rng(41)
    s = solver(fx, rng.standard_normal(fx.L))
    return fx, s, s.X, rng.standard_normal(fx.m), 0.7


def test_replay_on_a_fresh_solver():
    fx, s, X0, y, sigma = start()
    Ls = factors(81)
    tr, Lo = replay(s, fx, X0, y, y, Ls, sigma, 5)
    assert same_bits(s.X, X0)
    # lowrank_descent on the same start: the same recurrence with host sums in another order, so it agrees with the trace only within
    # the allowances above -- its f is lowrank_grad's, within 2 gamma(K_f) of c0 -- and a restart flag may differ where a slope lies
    # within its bound of 0.  Bit identity is not asserted; the first step has no sums in it and must agree on t to the quartic's data.
    de = s.lowrank_descent(Ls, y, sigma=sigma, steps=5)["trace"]
    Kg = grad_constants(fx, RANKS)
    fb = grad_twin(fx, X0, Ls, y, sigma)["fb"]
    assert len(de) == 5 and abs(LD(de[0]["f"]) - LD(tr[0, 6])) <= 2 * gamma(Kg["f"]) * fb
    assert same_bits(de[0]["t"], tr[0, 11]) and same_bits(de[0]["predicted"], tr[0, 12])      # step 0: D = -G bit for bit in both
    # the binding returns the same bits
    py = s.lowrank_refine(Ls, y, sigma, 5)
    assert py["steps"] == 5 and py["reason"] == 0 and len(py["trace"]) == 5
    assert all(same_bits(a, b) for a, b in zip(py["L"], Lo))
    assert all(same_bits([t[k] for k in TRACE[:13]], tr[i, :13]) for i, t in enumerate(py["trace"]))


def _traj(s):
    return [s.info_arr(k).copy() for k in INFO] + [s.X, s.y, s.S]


def test_replay_behind_a_solve_and_the_solve_continues():
    """a: 30 iterations, the call on the pending scaled state (ux = bscale), 30 more; b: the same without the call; d: 30 iterations and
    the getters, which the twins are evaluated at."""
    fx = fixture()
    a, b, d = (solver(fx) for _ in range(3))
    for s in (a, b, d):
        s.solve(30, 0.0)
    Ls = factors(61)
    replay(a, fx, d.X, d.y, None, Ls, 0.7, 5)
    for s in (a, b):
        s.solve(30, 0.0, if_first=False)
    for u, v in zip(_traj(a), _traj(b)):
        assert same_bits(u, v)
    assert a.info_iter_num == b.info_iter_num == 30
    # the getters before and after, in the caller's units now
    before = (a.X, a.y, a.S)
    a.lowrank_refine(Ls, None, 0.7, 2)
    assert all(same_bits(u, v) for u, v in zip(before, (a.X, a.y, a.S)))


def test_reasons():
    fx, s, X0, y, sigma = start()
    Ls = factors(83)
    Lv, rk = pack(BLK_A, Ls, RMAX)
    clean = flat(BLK_A, Ls, RMAX)
    # steps = 1
    rc, Lo, tr, o, _ = raw(s, Lv, rk, RMAX, y, sigma, 1, INF, 0.0)
    assert rc == 0 and o[0] == 1 and o[1] == 0 and tr[0, 5] == 1 and tr[0, 11] > 0
    five = raw(s, Lv, rk, RMAX, y, sigma, 5, INF, 0.0)
    assert same_bits(five[2][0, :13], tr[0, :13])
    # L_out may alias L_in
    al = Lv.copy()
    rc, Lo2, tr2, o2, _ = raw(s, al, rk, RMAX, y, sigma, 5, INF, 0.0, alias=True)
    assert rc == 0 and Lo2 is al and same_bits(al, five[1]) and same_bits(tr2[:, :13], five[2][:, :13])
    # gtol huge: no step, reason 2, the clean input back; the row holds the sums and the scalar update, no quartic
    rc, Lo, tr, o, _ = raw(s, Lv, rk, RMAX, y, sigma, 5, INF, 1e300)
    assert rc == 0 and o[0] == 0 and o[1] == 2 and same_bits(Lo, clean) and np.isnan(o[2]) and np.isnan(o[3]) and same_bits(o[4], np.sqrt(tr[0, 0]))
    assert same_bits(tr[0, :3], five[2][0, :3]) and np.all(tr[0, 6:13] == 0) and np.all(np.isnan(tr[1:]))
    # gtol = the first gradient norm that lies below every one before it: the loop stops there, before that step's line search
    gn = np.sqrt(five[2][:, 0])
    k = next((i for i in range(1, 5) if gn[i] < gn[:i].min()), None)
    print("gradient norms", gn, "first new minimum at step", k)
    if k is not None:
        rc, Lo, tr, o, _ = raw(s, Lv, rk, RMAX, y, sigma, 5, INF, gn[k])
        assert rc == 0 and o[1] == 2 and o[0] == k and same_bits(tr[:k, :13], five[2][:k, :13]) and same_bits(tr[k, :6], five[2][k, :6])
    # t_max tiny: every step ends at t_max and the descent is still monotone
    rc, Lo, tr, o, _ = raw(s, Lv, rk, RMAX, y, sigma, 3, 1e-9, 0.0)
    assert rc == 0 and o[0] == 3 and o[1] == 0 and np.all(tr[:, 11] == 1e-9) and np.all(tr[:, 12] < tr[:, 6])
    # sigma = 0 with t_max = inf: the quartic is a parabola in t that is not bounded below or has c3 = c4 = 0 and c2 <= 0 -- the
    # minimiser refuses, reason 4, or, where c2 > 0, the step is taken; either way the call returns 0 and the factors of the last step taken
    rc, Lo, tr, o, _ = raw(s, Lv, rk, RMAX, y, 0.0, 2, INF, 0.0)
    assert rc == 0 and o[1] in (0.0, 4.0) and np.all(tr[0, 9:11] == 0)
    if o[1] == 4:                                                            # at step k: the row has the coefficients and no t; the factors are those behind k steps
        k = int(o[0])
        assert k in (0, 1) and tr[k, 8] <= 0 and np.all(tr[k, 11:13] == 0) and np.all(np.isnan(tr[k + 1:]))
        assert same_bits(Lo, clean if k == 0 else raw(s, Lv, rk, RMAX, y, 0.0, k, INF, 0.0)[1])
        assert np.isnan(o[3]) if k == 0 else same_bits(o[3], tr[k - 1, 12])
    # D = 0 (a zero gradient): L = 0 on a problem whose gradient 2 S^ L vanishes there; finite t_max: t = 0, reason 1
    Z = [np.zeros(m.shape) for m in Ls]
    Zv, _ = pack(BLK_A, Z, RMAX)
    rc, Lo, tr, o, _ = raw(s, Zv, rk, RMAX, y, sigma, 4, 1.0, 0.0)
    assert rc == 0 and o[0] == 0 and o[1] == 1 and tr[0, 0] == 0 and tr[0, 11] == 0 and same_bits(Lo, np.zeros(Lo.size))
    rc, Lo, tr, o, _ = raw(s, Zv, rk, RMAX, y, sigma, 4, INF, 0.0)           # the constant quartic: t_max = inf is refused by the minimiser
    assert rc == 0 and o[0] == 0 and o[1] == 4
    assert same_bits(s.X, X0)


def test_ranks_zero_and_full_and_a_block_over_two_workgroups():
    """ranks 0 and n beside an unconstrained block; block 113, whose outer product is split over two workgroups"""
    blk, m = [113, -2, 40, 5], 12
    fx = make_opt_fixture(blk, m, 7)
    X0 = np.random.default_rng(3).standard_normal(fx.L)
    s = solver(fx, X0)
    y = np.random.default_rng(4).standard_normal(fx.m)
    for ranks, rmax in (((5, 0, 0, 5), 5), ((113, 0, 7, 0), 113)):
        replay(s, fx, X0, y, y, factors(5, ranks, blk, 0.3), 0.7, 3, blk, ranks, rmax, allowances=False)


BLK_I, M_I = [3, 20, -2, 33], 5


def test_calls_of_different_rmax_interleaved():
    fx = make_opt_fixture(BLK_I, M_I, 3)
    X0 = np.random.default_rng(91).standard_normal(fx.L)
    y = np.random.default_rng(92).standard_normal(fx.m)
    calls = (("refine", 4, (3, 4, 0, 0)), ("grad", 20, (0, 20, 0, 7)), ("refine", 33, (3, 0, 0, 33)), ("line", 1, (1, 0, 0, 1)), ("refine", 4, (3, 4, 0, 0)),
             ("refine", 20, (0, 20, 0, 13)))

    def call(s, i):
        name, rmax, ranks = calls[i]
        Fs, Ds = factors(700 + i, ranks, BLK_I, 0.5), factors(800 + i, ranks, BLK_I, 0.5)
        Lv, rk = pack(BLK_I, Fs, rmax)
        if name == "refine":
            rc, Lo, tr, o, r = raw(s, Lv, rk, rmax, y, 0.7, 3, 2.0, 0.0, m=fx.m)
            assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
            return [Lo, tr[:, :13], o[:5], r]
        if name == "grad":
            g = s.lowrank_grad(Fs, y, 0.7)
            return [flat(BLK_I, g["G"], rmax), g["r"], np.array([g["f"]])]
        ln = s.lowrank_line(Fs, Ds, y, 0.7, 2.0)
        return [ln["coef"], ln["r"], np.array([ln["t"], ln["f"]])]

    for iters in (0, 10):
        def fresh():
            s = solver(fx, X0)
            if iters:
                s.solve(iters, 0.0)
            return s
        one = fresh()
        got = [call(one, i) for i in range(len(calls))]
        for i in range(len(calls)):
            want = call(fresh(), i)
            assert len(want) == len(got[i]) and all(same_bits(a, b) for a, b in zip(got[i], want)), (iters, i)


def status_of(s):
    st = s.status()
    return {k: st[k] for k in st if k not in ("ms", "check_ms")}


def test_refusals_leave_the_solver_and_the_outputs_as_they_were():
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
        for L_, ranks_, rmax_, y_, sigma_, steps_, t_, g_ in ((Lv, ranks, RMAX, y, -0.5, 3, 1.0, 0.0), (Lv, ranks, RMAX, y, np.nan, 3, 1.0, 0.0), (Lv, ranks, RMAX, None, np.inf, 3, 1.0, 0.0),
                                                              (Lv, ranks, 0, y, 0.7, 3, 1.0, 0.0), (Lv, ranks, 8193, y, 0.7, 3, 1.0, 0.0), (Lv, None, RMAX, y, 0.7, 3, 1.0, 0.0),
                                                              (Lv, with_rank(1, -1), RMAX, y, 0.7, 3, 1.0, 0.0), (Lv, with_rank(2, 21), RMAX, y, 0.7, 3, 1.0, 0.0),
                                                              (Lv, with_rank(0, 4), RMAX, y, 0.7, 3, 1.0, 0.0), (None, ranks, RMAX, y, 0.7, 3, 1.0, 0.0),
                                                              (with_entry(2, 5, 69, np.nan), ranks, RMAX, y, 0.7, 3, 1.0, 0.0), (with_entry(4, 0, 0, np.inf), ranks, RMAX, None, 0.7, 3, 1.0, 0.0),
                                                              (Lv, ranks, RMAX, np.where(np.arange(fx.m) == 7, np.nan, y), 0.7, 3, 1.0, 0.0),
                                                              (Lv, ranks, RMAX, y, 0.7, 0, 1.0, 0.0), (Lv, ranks, RMAX, y, 0.7, -2, 1.0, 0.0),
                                                              (Lv, ranks, RMAX, y, 0.7, 3, 1.0, -1e-3), (Lv, ranks, RMAX, y, 0.7, 3, 1.0, np.nan),
                                                              (Lv, ranks, RMAX, y, 0.7, 3, 0.0, 0.0), (Lv, ranks, RMAX, y, 0.7, 3, -1.0, 0.0), (Lv, ranks, RMAX, y, 0.7, 3, np.nan, 0.0)):
            rc, Lo, tr, o, r = raw(s, L_, ranks_, rmax_, y_, sigma_, steps_, t_, g_)
            assert rc == -1 and all(np.all(np.isnan(v)) for v in (Lo, tr, o, r)), (rmax_, sigma_, steps_, t_, g_)      # CUADMM_ERR_INVALID, outputs untouched
            assert b"lowrank_refine" in lib.cuadmm_last_error()
        for want in ((False, True, True), (True, False, True), (True, True, False)):
            assert raw(s, Lv, ranks, RMAX, y, 0.7, 3, 1.0, 0.0, want=want)[0] == -1
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
    # not initialised; more than one rank
    fresh = cuadmm_amd.SDPSolver(verbose=False)
    assert raw(fresh, Lv, ranks, RMAX, y, 0.7, 3, 1.0, 0.0)[0] == -1
    w = cuadmm_amd.SDPSolver(verbose=False, rank=0, world=2)
    w.set_allreduce(lambda ptr, count, stream: None)
    w.init_problem(amd(fx))
    assert raw(w, Lv, ranks, RMAX, y, 0.7, 3, 1.0, 0.0)[0] == -1 and b"one rank" in lib.cuadmm_last_error()
    # the Python front end
    for args in ((Ls[:4], None, 0.5), (Ls, y[:-1], 0.5), (Ls, y, -1.0), (Ls, y, 0.5, 0), (Ls, y, 0.5, 3, 0.0), (Ls, y, 0.5, 3, 1.0, -1.0)):
        with pytest.raises(ValueError, match="lowrank_refine"):
            a.lowrank_refine(*args)
    # behind a failed cuadmm_update_A: CUADMM_ERR_FACTOR
    a.set_option("update_A_inject_fail", 1)                              # the test hook of tests/test_gpu_update_a.py
    with pytest.raises(cuadmm_amd.CuadmmError) as e:
        a.update_A(amd(fx).At_csc_vals * 1.5)
    assert e.value.code == -4
    rc, Lo, tr, o, r = raw(a, Lv, ranks, RMAX, y, 0.7, 3, 1.0, 0.0)
    assert rc == -4 and all(np.all(np.isnan(v)) for v in (Lo, tr, o, r)) and b"cuadmm_update_A" in lib.cuadmm_last_error()


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
    // the point of start_point() in the test: no solve, so that the state is the same in both front ends by construction
    std::vector<double> X0((size_t)problem.vec_len), S0((size_t)problem.vec_len), y0((size_t)problem.con_num);
    for (int i = 0; i < problem.vec_len; ++i) { X0[i] = (double)((i * 7) % 11 - 5) / 4.0; S0[i] = (double)((i * 5) % 13 - 6) / 8.0; }
    for (int j = 0; j < problem.con_num; ++j) y0[j] = (double)((j * 3) % 7 - 3) / 2.0;
    SDPSolver solver;
    solver.set_option("verbose", 0.0);
    solver.init(15, 30, problem.vec_len, problem.con_num, problem.At_csc_col_ptrs.data(), problem.At_csc_row_ids.data(), problem.At_csc_vals.data(),
                problem.At_nnz, problem.b_indices.data(), problem.b_vals.data(), problem.b_nnz, problem.C_indices.data(), problem.C_vals.data(),
                problem.C_nnz, blk_vals.data(), problem.mat_num, X0.data(), y0.data(), S0.data(), 1.0);
    const int rmax = 2;
    std::vector<int> ranks;
    std::vector<double> L;
    for (size_t k = 0; k < blk_vals.size(); ++k) {
      const int n = blk_vals[k];
      ranks.push_back(n > 0 ? 2 : 0);
      for (int t = 0; n > 0 && t < 2; ++t)
        for (int i = 0; i < n; ++i) L.push_back(((double)(i + 1) / (double)(t + 2) - (double)k) / 8.0);
    }
    const SDPSolver::LowRankRefine g = solver.lowrank_refine(L.data(), ranks.data(), rmax, nullptr, 0.7, 3);
    unsigned long long b0;
    std::printf("LRR %d %d %zu %zu %zu", g.steps, g.reason, g.L.size(), g.trace.size(), g.r.size());
    const double sc[3] = {g.f0, g.f, g.gnorm};
    for (double w : sc) { std::memcpy(&b0, &w, 8); std::printf(" %llx", b0); }
    for (double w : g.L) { std::memcpy(&b0, &w, 8); std::printf(" %llx", b0); }
    for (size_t e = 0; e < g.trace.size(); ++e)
      if (e % 16 < 13) { std::memcpy(&b0, &g.trace[e], 8); std::printf(" %llx", b0); }
    std::printf("\n");
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
    """The command line always solves first, so it is compared with the binding behind the same 40 iterations; the C++ facade at a point
    given to init (its solve ends with the deferred unscaling, the binding's leaves the scaled state pending).  The factors
    --lowrank-refine-out writes feed --start-lowrank."""
    fx = make_opt_fixture(BLK_C, M_C, 5)
    d, fdir, out = str(tmp_path / "prob") + "/", str(tmp_path / "factors") + "/", str(tmp_path / "refined") + "/"
    _write_txt(d, fx)
    os.makedirs(fdir)
    os.makedirs(out)
    Ls = [np.array([[((i + 1) / (t + 2) - k) / 8.0 for t in range(2)] for i in range(n)]) if n > 0 else np.zeros((0, 0)) for k, n in enumerate(BLK_C)]
    y1 = ((np.arange(M_C) * 5) % 9 - 4) / 8.0
    for k, n in enumerate(BLK_C):
        if n > 0:
            with open(fdir + "L_X_%d.txt" % k, "w") as f:
                f.write("".join("%.17g\n" % x for x in Ls[k].T.ravel()))
    libdir = os.path.join(ROOT, "cuadmm_amd", "lib")
    exe = os.path.join(libdir, "cuadmm_exe")
    for with_y, spec, t_max in ((False, "0.7,3", INF), (True, "0.7,3,2.5", 2.5)):
        if with_y:
            with open(fdir + "y.txt", "w") as f:
                f.write("".join("%.17g\n" % x for x in y1))
        s = cuadmm_amd.SDPSolver(verbose=False, profile=True)
        s.init_problem(cuadmm_amd.Problem.from_txt(d))
        s.solve(40, 0.0, 0, 50, 100, 5000, 1.05)
        py = s.lowrank_refine(Ls, y1 if with_y else None, 0.7, 3, t_max)
        js = str(tmp_path / ("lrr%d.json" % with_y))
        r = subprocess.run([exe, d, "--lowrank-refine=%s,%s" % (fdir, spec), "--lowrank-refine-out=" + out, "--max_iter=40", "--stop_tol=0", "--quiet", "--json=" + js],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.count(" lowrank_refine step ") == len(py["trace"]) and r.stdout.count(" lowrank_refine(sigma = 0.7") == 1
        with open(js) as f:
            side = json.load(f)["lowrank_refine"]
        assert side["sigma"] == 0.7 and side["rmax"] == 2 and side["y"] is with_y and side["max_steps"] == 3 and side["steps"] == py["steps"] and side["reason"] == py["reason"]
        assert side["f0"] == py["f0"] and side["f"] == py["f"] and side["gnorm"] == py["gnorm"]
        assert all(row[:13] == [float(t[k]) for k in TRACE[:13]] for row, t in zip(side["trace"], py["trace"])), with_y
        files = [np.array(open(out + "L_X_%d.txt" % k).read().split(), np.float64).reshape(2, n).T if n > 0 else np.zeros((0, 0)) for k, n in enumerate(BLK_C)]
        assert all(same_bits(a, b) for a, b in zip(files, py["L"])), with_y
    # the refined factors start a solve
    r = subprocess.run([exe, d, "--start-lowrank=" + out, "--max_iter=5", "--stop_tol=0", "--quiet"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " start(X): 3 blocks from factors, rank sum 6" in r.stdout, r.stderr[-2000:]
    # a directory without factor files, bad numbers, the output directory without the call: exit code 1 before any device work
    for args in (["--lowrank-refine=" + out + "none/"], ["--lowrank-refine=%s,-1" % fdir], ["--lowrank-refine=%s,0.7,0" % fdir], ["--lowrank-refine=%s,0.7,3,0" % fdir],
                 ["--lowrank-refine=%s,0.7,x" % fdir], ["--lowrank-refine-out=" + out]):
        r = subprocess.run([exe, d, "--quiet"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--lowrank-refine" in r.stderr, args
    # the C++ facade
    src, fexe = tmp_path / "facade.cpp", tmp_path / "facade"
    src.write_text(FACADE)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(fexe), "-L" + libdir,
                           "-lcuadmm_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"], timeout=300)
    r = subprocess.run([str(fexe), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("LRR ")]
    assert len(lines) == 1
    prob = cuadmm_amd.Problem.from_txt(d)
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(prob, *start_point(prob.vec_len, prob.con_num))
    py = s.lowrank_refine(Ls, None, 0.7, 3)
    ln = lines[0]
    nL = lowrank_size(BLK_C, 2)
    assert [int(x) for x in ln[1:6]] == [py["steps"], py["reason"], nL, 16 * len(py["trace"]), M_C]
    want = np.concatenate([[py["f0"], py["f"], py["gnorm"]], np.concatenate([m.T.ravel() for m in py["L"]]),
                           np.concatenate([[t[k] for k in TRACE[:13]] for t in py["trace"]])])
    assert [int(x, 16) for x in ln[6:]] == [int(b) for b in bits(want)]
