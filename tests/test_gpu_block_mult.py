"""Blocks times factors on the GPU (include/cuadmm_amd.h: cuadmm_block_multiply, cuadmm_op_block_mult; csrc/block_mult.h; DESIGN.md, "Blocks
times factors"): the kernel W_k = M_k V_k on every tile edge, n mod 4, rank class and sign through the op hook, then the solver entry
(the kernel's bits on a fresh solver, the scaled iterate behind a solve, <X, S> through the factors, C - A'y, the host sums, the solve
that continues bit for bit, refusals) and the three front ends.

Tolerances, none of them measured (u = 2^-53).  The kernel: its contract |W - exact| <= (n + 4) u |M| |V| against the np.longdouble
reference of tests/_block_mult_twin.py, and bit-exact results where the arithmetic is exact (small integers, fractions.Fraction).  Behind a
solve two more u: the unit applied to W on the host, and the reference's matrix, which is the getter's rounded product of the same unit.
C - A'y: see test_dual_matrix_against_longdouble.  Everything else is compared bit for bit."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd.devbuf import Dev
from tests._block_mult_twin import LD, U, exact, host_sums, loffs, lowrank_size, matrix, offsets, pack, reference, unpack
from tests._lower_bound_twin import make_opt_fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
BLK_OP = [1, 2, 3, 15, 16, 17, -2, 31, 32, 33, 64, 65, 130, -5, 300]
RANK_SET = (0, 1, 3, 4, 5, 16, 17, 10 ** 6)      # the last: min(n, rmax)
BLK_A, M_A = [3, 20, 70, -2, 130], 40          # the small fixture of tests/test_gpu_lowrank.py
INFO = ("pobj", "dobj", "errRp", "errRd", "relgap", "sig", "bscale", "Cscale")
WHICH = ("X", "S", "dual")
_fx = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def op(blk, vec, Vs, rmax, sign=1.0, check_input=True):
    """the (n_k, r_k) products cuadmm_op_block_mult returns: V padded with NaN in every unread column, W pre-filled with NaN; asserts
    that the padding of W is + 0.0 and that the device vector keeps its bits"""
    lib = cuadmm_amd.load()
    V, ranks = pack(blk, Vs, rmax)
    W = np.full(V.size, np.nan)
    b = np.asarray(blk, np.int32)
    vec = np.ascontiguousarray(vec, np.float64)
    d = Dev(vec)
    rc = lib.cuadmm_op_block_mult(d.ptr, P(b), b.size, float(sign), P(V), P(ranks), rmax, P(W), None)
    assert rc == 0, lib.cuadmm_last_error()
    if check_input:
        assert same_bits(d.get(), vec)
    assert not np.any(np.isnan(W[:lowrank_size(blk, rmax)]))
    Ws, pads = unpack(blk, ranks, rmax, W)
    for k, pad in enumerate(pads):
        assert same_bits(pad, np.zeros(pad.size)), (k, "padding of W")
    return Ws


def check(blk, vec, Vs, Ws, sign, is_exact, spare=0):
    off = offsets(blk)
    for k, n in enumerate(blk):
        if n < 0:
            assert Ws[k].shape == (0, 0)
            continue
        seg, V, W = vec[off[k]:off[k + 1]], Vs[k], Ws[k]
        assert W.shape == V.shape
        if V.shape[1] == 0:
            continue
        if is_exact:
            want = exact(seg, n, V, sign)
            assert same_bits(W, want), (k, n, V.shape[1], np.argwhere(bits(W) != bits(want))[:4].tolist())
            continue
        ref, A = reference(seg, n, V, sign)
        err = np.abs(W.astype(LD) - ref)
        bound = (n + 4 + spare) * LD(U) * A
        worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        assert np.all(err <= bound), (k, n, V.shape[1], worst, float(err[worst]), float(bound[worst]))


def data(blk, ranks, rng, is_exact):
    off = offsets(blk)
    if is_exact:
        vec = rng.integers(-3, 4, size=int(off[-1])).astype(np.float64)
        Vs = [rng.integers(-3, 4, size=(max(n, 0), r if n > 0 else 0)).astype(np.float64) for n, r in zip(blk, ranks)]
    else:
        vec = rng.standard_normal(int(off[-1])) * np.exp(rng.uniform(-2, 2, size=int(off[-1])))
        Vs = [rng.standard_normal((max(n, 0), r if n > 0 else 0)) * np.exp(rng.uniform(-3, 3, size=(1, r if n > 0 else 0))) for n, r in zip(blk, ranks)]
    return vec, Vs


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------
# rmax = 300: every rank of the set up to r = n on every size (several passes of 64 columns at n = 65, 130, 300); rmax = 20 < n from 31
# on: the block's range in V / W is min(n, rmax) columns wide, ranks 16 and 17 fit; rmax = 6: the capped rank is min(n, 6)
@pytest.mark.parametrize("is_exact", [False, True], ids=["contract", "integers"])
@pytest.mark.parametrize("rmax", [300, 20, 6])
def test_kernel_on_every_edge(rmax, is_exact):
    """Eight calls: block k of call q takes rank RANK_SET[(k + q) % 8] capped at min(n, rmax), so that every block meets every rank of
    the set; the sign alternates from call to call.  The second call is repeated: the same bits from run to run."""
    rng = np.random.default_rng(rmax + 7 * is_exact)
    for q in range(len(RANK_SET)):
        ranks = [min(RANK_SET[(k + q) % len(RANK_SET)], n, rmax) if n > 0 else 0 for k, n in enumerate(BLK_OP)]
        sign = 1.0 if q % 2 == 0 else -1.0
        vec, Vs = data(BLK_OP, ranks, rng, is_exact)
        Ws = op(BLK_OP, vec, Vs, rmax, sign)
        check(BLK_OP, vec, Vs, Ws, sign, is_exact)
        if q == 1:
            again = op(BLK_OP, vec, Vs, rmax, sign)
            assert all(same_bits(a, b) for a, b in zip(Ws, again))


def test_kernel_refuses_bad_ranks_before_the_device():
    lib = cuadmm_amd.load()
    blk = np.array([5, -2, 40], np.int32)
    d = Dev(np.full(15 + 2 + 820, 3.0))
    V = np.ones(lowrank_size(blk, 8))
    W = np.full(V.size, 7.0)
    for ranks, rmax in (([6, 0, 1], 8), ([1, 0, 9], 8), ([-1, 0, 1], 8), ([1, 0, 1], 0), ([1, 0, 1], 8193)):
        assert lib.cuadmm_op_block_mult(d.ptr, P(blk), 3, 1.0, P(V), P(np.array(ranks, np.int32)), rmax, P(W), None) == -1, (ranks, rmax)
    assert lib.cuadmm_op_block_mult(d.ptr, P(blk), 3, 1.0, None, P(np.array([0, 0, 1], np.int32)), 8, P(W), None) == -1
    assert np.all(W == 7.0) and np.all(d.get() == 3.0)
    # every rank 0 needs no V: + 0.0 everywhere
    assert lib.cuadmm_op_block_mult(d.ptr, P(blk), 3, 1.0, None, P(np.array([0, 9, 0], np.int32)), 8, P(W), None) == 0
    assert same_bits(W, np.zeros(W.size))


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


def fixture_factors(seed, ranks=(2, 5, 7, 0, 16)):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((max(n, 0), r if n > 0 else 0)) for n, r in zip(BLK_A, ranks)]


def raw(s, which, V, ranks, rmax, W=True, out=True, pb=True):
    """(rc, W buffer, out8, per_block) of cuadmm_block_multiply; the outputs pre-filled with NaN"""
    Wb = np.full(max(lowrank_size(BLK_A, max(min(rmax, 8192), 1)), 1), np.nan) if W else None
    o = np.full(8, np.nan) if out else None
    p = np.full(4 * len(BLK_A), np.nan) if pb else None
    rc = cuadmm_amd.load().cuadmm_block_multiply(s._h, which, P(V), P(ranks), rmax, P(Wb), P(o), P(p))
    return rc, Wb, o, p


def _traj(s):
    return [s.info_arr(k).copy() for k in INFO] + [s.X, s.y, s.S]


@pytest.mark.parametrize("which", [0, 1])
def test_fresh_solver_returns_the_kernels_bits(which):
    fx = fixture()
    s = solver(fx, fx.Xs, fx.ys, fx.Ss)
    rmax = 20                                                               # < 70, 130: the ranges are 20 columns wide
    Vs = fixture_factors(3 + which)
    V, ranks = pack(BLK_A, Vs, rmax)
    rc, W, o, pb = raw(s, which, V, ranks, rmax)
    assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
    Ws, pads = unpack(BLK_A, ranks, rmax, W)
    want = op(BLK_A, (s.X, s.S)[which], Vs, rmax)
    assert all(same_bits(a, b) for a, b in zip(Ws, want)) and all(same_bits(p, np.zeros(p.size)) for p in pads)
    # per_block and out8 from the returned W, bit for bit
    tpb, to = host_sums(BLK_A, Vs, Ws)
    assert same_bits(pb.reshape(-1, 4), tpb) and same_bits(o[:6], to)
    assert o[2] in (0, 1, 2, 4) and o[4] == 4 and o[5] == 30 and o[6] > 0 and o[7] >= 16 * lowrank_size(BLK_A, rmax)
    # per_block may be null; every rank 0 and no V: + 0.0 and zeros
    assert raw(s, which, V, ranks, rmax, pb=False)[0] == 0
    rc, W, o, pb = raw(s, which, None, np.zeros(5, np.int32), 1)
    assert rc == 0 and same_bits(W, np.zeros(W.size)) and same_bits(o[:6], np.array([0.0, 0.0, 0.0, 0.0, 4.0, 0.0]))
    assert pb.reshape(-1, 4).tolist() == [[0, 0, 0, 0]] * 3 + [[0, 0, 0, 2]] + [[0, 0, 0, 0]]
    # the Python front end returns the same arrays
    r = s.block_multiply(WHICH[which], Vs)
    assert all(same_bits(a, b) for a, b in zip(r["W"], want)) and same_bits(r["per_block"], tpb) and r["rank_sum"] == 30 and r["blocks"] == 4


def _against_numpy(Ws, vec, Vs, spare, extra=None):
    """|W - M V| <= (n + 4 + spare) u |M| |V| (+ extra_k, an (n, r) array) for the matrix of vec in longdouble"""
    off = offsets(BLK_A)
    for k, n in enumerate(BLK_A):
        if n < 0 or Vs[k].shape[1] == 0:
            continue
        ref, A = reference(vec[off[k]:off[k + 1]], n, Vs[k])
        err = np.abs(Ws[k].astype(LD) - ref)
        bound = (n + 4 + spare) * LD(U) * A + (0 if extra is None else extra[k])
        worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        print("block", k, "n", n, "max err / bound %.3f" % float(np.max(err / np.maximum(bound, LD(1e-300)))))
        assert np.all(err <= bound), (k, n, worst, float(err[worst]), float(bound[worst]))


def test_behind_a_solve_the_scaled_iterate_is_read():
    """a: the getters (they run the deferred unscaling).  b: block_multiply on the pending scaled state, nothing before it."""
    fx = fixture()
    a, b = solver(fx), solver(fx)
    for s in (a, b):
        s.solve(30, 0.0)
    Vs = fixture_factors(11, ranks=(3, 4, 9, 0, 12))
    got = {w: b.block_multiply(w, Vs) for w in ("X", "S")}                  # before any getter of b
    for w, vec in (("X", a.X), ("S", a.S)):
        _against_numpy(got[w]["W"], vec, Vs, 2)
        tpb, to = host_sums(BLK_A, Vs, got[w]["W"])
        assert same_bits(got[w]["per_block"], tpb)
        assert same_bits(np.array([got[w][k] for k in ("norm", "inner", "block", "block_norm", "blocks", "rank_sum")], np.float64), to)
    for u, v in zip((b.X, b.y, b.S), (a.X, a.y, a.S)):
        assert same_bits(u, v)


ITERS_XS = 400          # far enough into the solve for the factor's residual, the largest term of the tolerance, to be small


def test_complementarity_through_the_factors():
    """sum_k <L_k, (S L)_k> against evaluate()'s <X, S>, L = lowrank("X", tol = 0).  Three contracts add up:
    the factor's, ||X_k - L_k L_k'||_F <= resid_k + 4 (n + 2) u tr X_k (tests/_lowrank_twin.py; 4 u tr X_k more for the rounded
    sqrt(unit) on L behind a solve), times ||S_k||_F; the product's, (n + 6) u |L|' |S| |L| summed, with the host's sequential sum over
    n r terms, n r u sum |L| |W|; and the evaluation's sum over vec_len products in some order, (vec_len + 8) u sum |X_i| |S_i|.  The
    evaluation's sum runs over the unconstrained blocks too: their part, from the getters of a second solver, is taken off."""
    fx = fixture()
    a, b = solver(fx), solver(fx)
    for s in (a, b):
        s.solve(ITERS_XS, 0.0)
    ev = b.evaluate()
    f = b.lowrank("X", tol=0.0)
    r = b.block_multiply("S", f["L"])
    Xa, Sa = a.X, a.S
    off = offsets(BLK_A)
    tol = (len(Xa) + 8) * U * float(np.sum(np.abs(Xa) * np.abs(Sa)))
    for k, n in enumerate(BLK_A):
        if n < 0:
            continue
        Lk = np.abs(f["L"][k].astype(LD))
        nS = float(np.linalg.norm(Sa[off[k]:off[k + 1]]))
        tol += (f["resid"][k] + (4 * (n + 2) + 4) * U * f["trace"][k]) * nS
        tol += (n + 6) * U * float(np.sum(Lk * (np.abs(matrix(Sa[off[k]:off[k + 1]], n)) @ Lk)))
        tol += n * Lk.shape[1] * U * float(np.sum(Lk * np.abs(r["W"][k])))
    free = sum(float(np.sum(Xa[off[k]:off[k + 1]].astype(LD) * Sa[off[k]:off[k + 1]].astype(LD))) for k, n in enumerate(BLK_A) if n < 0)
    diff = abs(ev["XS"] - free - r["inner"])
    print("<X,S> evaluate %.6e (unconstrained part %.3e), through the factors %.6e, difference %.3e, tolerance %.3e" % (ev["XS"], free, r["inner"], diff, tol))
    assert diff <= tol


def test_dual_matrix_with_y_zero_is_C():
    fx = fixture()
    s = solver(fx)                                                          # y = 0
    Vs = fixture_factors(17)
    r = s.block_multiply("dual", Vs)
    _against_numpy(r["W"], fx.C, Vs, 2)                                     # C / Cscale and the unit on W: two more u
    assert r["blocks"] == 4 and r["ms"] > 0


def test_dual_matrix_against_longdouble():
    """S^ = C - A'y in longdouble from the fixture's arrays.  The engine forms slot i in its scaled space (csrc/vec_kernels.hip:
    aty_xb_kernel, csrc/engine_reports.hip: stage_scaled_y, bm_run) as t - C_i / Cscale, t = sum_j (A_ji / normA_j) ((y_j normA_j) ics)
    over the c_i entries of row i of A', ics = fl(1 / Cscale), and W takes the unit Cscale on the host.  Roundings on a term of the sum:
    A_ji / normA_j 1, ics 1, the two products on y 2, the product 1, at most c_i additions (the subtraction of C among them, in either
    of the two kernels' orders), the unit 1: c_i + 6.  On C_i: ics 1, its product 1, the subtraction 1, the unit 1: 4.  So slot i is
    within gamma(c_i + 6) (|C_i| + (|A|'|y|)_i), gamma(k) = k u / (1 - k u), of the exact one -- inside the (c_i + 12) u the 12 of which
    covers the scalings -- and that allowance goes through |V| as the slots do: / sqrt(2) off the diagonal.  The product itself: (n + 4) u
    on the matrix that was formed, whose entries are within the allowance of the exact ones; one spare u for that second-order term."""
    fx = fixture()
    rng = np.random.default_rng(23)
    y = rng.standard_normal(fx.m)
    s = solver(fx)
    s.set_XyS(y=y)
    Vs = fixture_factors(19, ranks=(3, 20, 6, 0, 9))
    r = s.block_multiply("dual", Vs)
    Al = fx.A.astype(LD)
    Sh = fx.C.astype(LD) - Al.T @ y.astype(LD)
    c = np.count_nonzero(fx.A, axis=0)
    kk = (c + 6) * LD(U)
    slot = kk / (1 - kk) * (np.abs(fx.C).astype(LD) + np.abs(Al).T @ np.abs(y).astype(LD))
    off = offsets(BLK_A)
    extra = {}
    for k, n in enumerate(BLK_A):
        if n > 0:
            E = matrix(slot[off[k]:off[k + 1]], n)                          # the allowance as a matrix: slots / sqrt(2) off the diagonal
            extra[k] = (1 + (n + 5) * LD(U)) * (E @ np.abs(Vs[k]).astype(LD))
    _against_numpy(r["W"], Sh, Vs, 1, extra)
    # the same y through lambda_min's route: the calls share nothing but the auxiliary input vector
    assert np.isfinite(s.lambda_min("dual")["lambda_min"])
    again = s.block_multiply("dual", Vs)
    assert all(same_bits(u, v) for u, v in zip(again["W"], r["W"]))


def test_a_solve_continues_bit_for_bit():
    fx = fixture()
    a, b = solver(fx), solver(fx)
    Vs = fixture_factors(29)
    for s in (a, b):
        s.solve(30, 0.0)
    for w in WHICH:
        assert a.block_multiply(w, Vs)["blocks"] == 4
    for s in (a, b):
        s.solve(30, 0.0, if_first=False)
    for u, v in zip(_traj(a), _traj(b)):
        assert same_bits(u, v)
    assert a.info_iter_num == b.info_iter_num == 30


def test_refusals_leave_the_solver_as_it_was():
    fx = fixture()
    lib = cuadmm_amd.load()
    a, b = solver(fx), solver(fx)
    for s in (a, b):
        s.solve(20, 0.0)
    rmax = 16
    Vs = fixture_factors(31)
    V, ranks = pack(BLK_A, Vs, rmax)
    lo = loffs(BLK_A, rmax)

    def with_rank(k, r):
        q = ranks.copy()
        q[k] = r
        return q

    def with_entry(k, col, row, x):
        q = V.copy()
        q[lo[k] + col * BLK_A[k] + row] = x
        return q

    def refused(s):
        for args in ((-1, V, ranks, rmax), (3, V, ranks, rmax), (0, V, ranks, 0), (2, V, ranks, 8193), (0, V, None, rmax),
                     (0, V, with_rank(1, -1), rmax), (1, V, with_rank(2, 17), rmax), (2, V, with_rank(0, 4), rmax), (1, None, ranks, rmax),
                     (0, with_entry(2, 6, 69, np.nan), ranks, rmax), (1, with_entry(4, 0, 0, np.inf), ranks, rmax), (2, with_entry(1, 4, 19, -np.inf), ranks, rmax)):
            rc, W, o, pb = raw(s, *args)
            assert rc == -1 and np.all(np.isnan(o)) and np.all(np.isnan(W)) and np.all(np.isnan(pb)), args[0]      # CUADMM_ERR_INVALID, outputs untouched
            assert "block_multiply" in lib.cuadmm_last_error().decode()
        assert raw(s, 0, V, ranks, rmax, W=False)[0] == -1 and raw(s, 0, V, ranks, rmax, out=False)[0] == -1
    # a NaN in a column that is not read is no reason to refuse (block 2 has 7 columns: column 7 is not one of them)
    assert np.isnan(V[lo[2] + 7 * 70])
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
    assert raw(fresh, 0, V, ranks, rmax)[0] == -1
    w = cuadmm_amd.SDPSolver(verbose=False, rank=0, world=2)
    w.set_allreduce(lambda ptr, count, stream: None)
    w.init_problem(amd(fx))
    assert raw(w, 0, V, ranks, rmax)[0] == -1 and "one rank" in lib.cuadmm_last_error().decode()
    blk_g = [6, 10, 6, 10]                                                  # (the duo front end takes two block sizes)
    p = amd(make_opt_fixture(blk_g, 8, 9))
    g = cuadmm_amd.SDPSolver(verbose=False, options={"duo_share_device": 1})
    g.duo_init(True, 2, 15, 30, p.vec_len, p.con_num, p.At_csc_col_ptrs, p.At_csc_row_ids, p.At_csc_vals, p.At_nnz, p.b_indices, p.b_vals, p.b_nnz,
               p.C_indices, p.C_vals, p.C_nnz, p.blk_vals, p.mat_num)
    assert g.group_info()["engines"] == 2
    Vg, rg = pack(blk_g, [np.ones((n, 2)) for n in blk_g], 2)
    Xg = g.X
    o = np.full(8, np.nan)
    assert lib.cuadmm_block_multiply(g._h, 0, P(Vg), P(rg), 2, P(np.zeros(Vg.size)), P(o), None) == -1 and "one rank" in lib.cuadmm_last_error().decode()
    assert same_bits(g.X, Xg)
    # the Python front end: a wrong row count, a wrong number of entries, a wrong name
    bad = [m.copy() for m in Vs]
    bad[1] = np.zeros((19, 2))
    for arg in (bad, Vs[:4]):
        with pytest.raises(ValueError, match="block_multiply"):
            a.block_multiply("X", arg)
    with pytest.raises(ValueError):
        a.block_multiply("y", Vs)
    # behind a failed cuadmm_update_A: X and S are still multiplied, the dual matrix is refused with CUADMM_ERR_FACTOR
    a.set_option("update_A_inject_fail", 1)                              # the test hook of tests/test_gpu_update_a.py
    with pytest.raises(cuadmm_amd.CuadmmError) as e:
        a.update_A(amd(fx).At_csc_vals * 1.5)
    assert e.value.code == -4
    assert raw(a, 0, V, ranks, rmax)[0] == 0 and raw(a, 1, V, ranks, rmax)[0] == 0
    rc, W, o, pb = raw(a, 2, V, ranks, rmax)
    assert rc == -4 and np.all(np.isnan(o)) and np.all(np.isnan(W)) and "cuadmm_update_A" in lib.cuadmm_last_error().decode()


def status_of(s):
    st = s.status()
    return {k: st[k] for k in st if k not in ("ms", "check_ms")}


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
    std::vector<double> X0((size_t)problem.vec_len), S0((size_t)problem.vec_len), y0((size_t)problem.con_num);
    for (int i = 0; i < problem.vec_len; ++i) { X0[i] = (double)((i * 7) % 11 - 5) / 4.0; S0[i] = (double)((i * 5) % 13 - 6) / 8.0; }
    for (int j = 0; j < problem.con_num; ++j) y0[j] = (double)((j * 3) % 7 - 3) / 2.0;
    SDPSolver solver;
    solver.set_option("verbose", 0.0);
    solver.init(15, 30, problem.vec_len, problem.con_num, problem.At_csc_col_ptrs.data(), problem.At_csc_row_ids.data(), problem.At_csc_vals.data(),
                problem.At_nnz, problem.b_indices.data(), problem.b_vals.data(), problem.b_nnz, problem.C_indices.data(), problem.C_vals.data(),
                problem.C_nnz, blk_vals.data(), problem.mat_num, X0.data(), y0.data(), S0.data(), 1.0);
    // V: two columns per PSD block, entry (row i, column t) of block k = (i + 1) / (t + 2) - k
    const int rmax = 2;
    std::vector<int> ranks;
    std::vector<double> V;
    for (size_t k = 0; k < blk_vals.size(); ++k) {
      const int n = blk_vals[k];
      ranks.push_back(n > 0 ? 2 : 0);
      for (int t = 0; n > 0 && t < 2; ++t)
        for (int i = 0; i < n; ++i) V.push_back((double)(i + 1) / (double)(t + 2) - (double)k);
    }
    for (int which = 0; which < 3; ++which) {
      const SDPSolver::BlockMultiply r = solver.block_multiply(which, V.data(), ranks.data(), rmax);
      unsigned long long b0, b1;
      std::memcpy(&b0, &r.norm, 8);
      std::memcpy(&b1, &r.inner, 8);
      std::printf("BM %d %llx %llx %d %d %.0f %zu", which, b0, b1, r.block, r.blocks, r.rank_sum, r.W.size());
      for (double w : r.W) { std::memcpy(&b0, &w, 8); std::printf(" %llx", b0); }
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
    """The command line always solves first, so it is compared with the binding behind the same 40 iterations.  The C++ facade is
    compared with the binding at a point given to init (start_point): SDPSolver::solve of include/cuadmm_amd.hpp ends with fetch(), which
    reads X, y, S and so runs the deferred unscaling, while the binding's solve leaves the scaled state pending.  Behind a solve the facade
    therefore multiplies the unscaled X (unit 1) and the binding the scaled one with the unit on W: the same product to (n + 6) u, as
    test_behind_a_solve_the_scaled_iterate_is_read checks, but not the same bits.  At a point given to init both hold the same vectors."""
    fx = make_opt_fixture(BLK_C, M_C, 5)
    d, fdir, out = str(tmp_path / "prob") + "/", str(tmp_path / "factors") + "/", str(tmp_path / "w") + "/"
    _write_txt(d, fx)
    os.makedirs(fdir)
    os.makedirs(out)
    Vs = [np.array([[(i + 1) / (t + 2) - k for t in range(2)] for i in range(n)]) if n > 0 else np.zeros((0, 0)) for k, n in enumerate(BLK_C)]
    for k, n in enumerate(BLK_C):
        if n > 0:
            with open(fdir + "L_X_%d.txt" % k, "w") as f:
                f.write("".join("%.17g\n" % x for x in Vs[k].T.ravel()))
    with open(fdir + "L_S_1.txt", "w") as f:                                # does not fit its block, and is not opened: the factors of X are used
        f.write("1.0\n")
    libdir = os.path.join(ROOT, "cuadmm_amd", "lib")
    # the binding
    s = cuadmm_amd.SDPSolver(verbose=False, profile=True)
    s.init_problem(cuadmm_amd.Problem.from_txt(d))
    s.solve(40, 0.0, 0, 50, 100, 5000, 1.05)
    py = {w: s.block_multiply(w, Vs) for w in WHICH}
    # the command line: the last --block-mult writes the files
    side = {}
    files = {}
    for w in WHICH:
        js = str(tmp_path / ("%s.json" % w))
        r = subprocess.run([os.path.join(libdir, "cuadmm_exe"), d, "--block-mult=%s,%s" % (w, fdir), "--block-mult-out=" + out, "--max_iter=40", "--stop_tol=0",
                            "--quiet", "--json=" + js], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.count(" block_mult(%s): " % w) == 1
        with open(js) as f:
            side[w] = json.load(f)["block_mult"]
        files[w] = [np.array(open(out + "W_%d.txt" % k).read().split(), np.float64).reshape(2, n).T if n > 0 else np.zeros((0, 0)) for k, n in enumerate(BLK_C)]
    for w in WHICH:
        assert len(side[w]) == 1 and side[w][0]["which"] == w and side[w][0]["rmax"] == 2
        for key in ("norm", "inner", "block", "block_norm", "blocks", "rank_sum"):
            assert side[w][0][key] == py[w][key], (w, key)
        assert all(same_bits(a, b) for a, b in zip(files[w], py[w]["W"])), w
    # a directory without factor files: exit code 1 before any device work
    r = subprocess.run([os.path.join(libdir, "cuadmm_exe"), d, "--block-mult=S," + out + "none/", "--quiet"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--block-mult" in r.stderr
    # the C++ facade
    src, fexe = tmp_path / "facade.cpp", tmp_path / "facade"
    src.write_text(FACADE)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(fexe), "-L" + libdir,
                           "-lcuadmm_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"], timeout=300)
    r = subprocess.run([str(fexe), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("BM ")]
    assert len(lines) == 3
    prob = cuadmm_amd.Problem.from_txt(d)
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(prob, *start_point(prob.vec_len, prob.con_num))
    py = {w: s.block_multiply(w, Vs) for w in WHICH}
    for ln in lines:
        w = WHICH[int(ln[1])]
        as_bits = lambda x: int(np.float64(x).view(np.uint64))
        assert int(ln[2], 16) == as_bits(py[w]["norm"]) and int(ln[3], 16) == as_bits(py[w]["inner"])
        assert int(ln[4]) == py[w]["block"] and int(ln[5]) == 3 and int(ln[6]) == 6 and int(ln[7]) == lowrank_size(BLK_C, 2)
        flat = np.concatenate([m.T.ravel() for m in py[w]["W"]])
        assert [int(x, 16) for x in ln[8:]] == [int(b) for b in bits(flat)]
