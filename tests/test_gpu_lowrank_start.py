"""Start from per-block low-rank factors on the GPU (include/cuadmm_amd.h: cuadmm_set_lowrank, cuadmm_op_block_outer; csrc/lowrank_apply.h;
DESIGN.md, "Starting from low-rank factors"): the kernel svec(L_k L_k') on every size class, tile edge and K-padding edge through the op
hook, then the solver entry (the kernel's bits where they belong and nothing else touched, on a fresh solver and behind a solve; the
equivalence with cuadmm_set_XyS; the round trip through cuadmm_lowrank; refusals; out4) and the three front ends.

Tolerances, none of them measured.  The kernel: its rounding contract |computed - exact| <= (r + 4) u c_ij sum_t |L_it| |L_jt| against a
np.longdouble reference (whose own error, (r + 1) 2^-64 of the same sum, is far inside the two spare u), and bit-exact results where the
arithmetic is exact (small-integer L).  The round trip: the sum of the factor's contract (tests/_lowrank_twin.py: ||M - L L'||_F <= resid +
4 (n + 2) u tr M) and the kernel's.  Everything else is compared bit for bit."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd.devbuf import Dev
from tests._lower_bound_twin import blk_lens, make_opt_fixture
from tests._lowrank_twin import U, lowrank_size

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
LD = np.longdouble
SQRT2 = 1.4142135623730951                       # kLoSqrt2 (csrc/lowrank_apply.h)
BLK_A, M_A = [3, 20, 70, -2, 130], 40          # fixture A of tests/test_gpu_lowrank.py
INFO = ("pobj", "dobj", "errRp", "errRd", "relgap", "sig", "bscale", "Cscale")
SENTINEL = np.array([0x7FF8DEADBEEF0001, 0xFFF0000000000000, 0x8000000000000000, 0x0000000000000001], np.uint64).view(np.float64)
_fx = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def offsets(blk):
    return np.concatenate([[0], np.cumsum(blk_lens(blk))])


def pack_nan(blk, Ls, rmax):
    """the factor buffer for rmax with NaN in every column that must not be read, and the ranks"""
    L = np.full(max(lowrank_size(blk, rmax), 1), np.nan)
    ranks = np.zeros(len(blk), np.int32)
    at = 0
    for k, n in enumerate(blk):
        if n <= 0:
            ranks[k] = 77                                                    # ignored
            continue
        r = Ls[k].shape[1]
        L[at:at + n * r] = Ls[k].T.ravel()
        ranks[k] = r
        at += n * min(n, rmax)
    return L, ranks


def op(blk, Ls, rmax, vec):
    """the vector cuadmm_op_block_outer leaves"""
    lib = cuadmm_amd.load()
    L, ranks = pack_nan(blk, Ls, rmax)
    b = np.asarray(blk, np.int32)
    d = Dev(np.asarray(vec, np.float64))
    rc = lib.cuadmm_op_block_outer(P(L), P(ranks), P(b), b.size, rmax, d.ptr, None)
    assert rc == 0, lib.cuadmm_last_error()
    return d.get()


def prefilled(blk):
    """NaN in every PSD slot, the sentinel bits in the slots of the unconstrained blocks"""
    off = offsets(blk)
    v = np.full(int(off[-1]), np.nan)
    for k, n in enumerate(blk):
        if n < 0:
            v[off[k]:off[k + 1]] = np.resize(SENTINEL, -n)
    return v


def check_blocks(blk, Ls, got, exact):
    off = offsets(blk)
    for k, n in enumerate(blk):
        g = got[off[k]:off[k + 1]]
        if n < 0:
            assert same_bits(g, np.resize(SENTINEL, -n)), (k, n)           # not touched
            continue
        Lk = Ls[k]
        r = Lk.shape[1]
        assert not np.any(np.isnan(g)), (k, n, r, "a slot was not written or an unread column leaked")
        ii, jj = np.tril_indices(n)
        if r == 0:
            assert same_bits(g, np.zeros(g.size)), (k, n)                   # + 0.0
            continue
        if exact:                                                            # small integers: every product and sum is exact
            G = (Lk.astype(np.int64) @ Lk.astype(np.int64).T)[ii, jj].astype(np.float64)
            want = np.where(ii == jj, G, np.float64(SQRT2) * G)
            assert same_bits(g + 0.0, want + 0.0), (k, n, r, np.flatnonzero(g != want)[:5])
            continue
        Ll = Lk.astype(LD)
        G = (Ll @ Ll.T)[ii, jj]
        A = (np.abs(Ll) @ np.abs(Ll).T)[ii, jj]
        c = np.where(ii == jj, LD(1), np.sqrt(LD(2)))
        err = np.abs(g.astype(LD) - c * G)
        bound = (r + 4) * LD(U) * c * A
        worst = int(np.argmax(err - bound))
        assert np.all(err <= bound), (k, n, r, (int(ii[worst]), int(jj[worst])), float(err[worst]), float(bound[worst]))


def factors(blk, ranks, rng, exact):
    out = []
    for n, r in zip(blk, ranks):
        if n < 0:
            out.append(np.zeros((0, 0)))
        elif exact:
            out.append(rng.integers(-3, 4, size=(n, r)).astype(np.float64))
        else:
            out.append(rng.standard_normal((n, r)) * np.exp(rng.uniform(-3, 3, size=(1, r))))
    return out


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 130)      # tile edges of the three paths: one wavefront (<= 32), one workgroup


def small_list(rmax):
    """every size crossed with r in {0, 1, 3, 4, 5, n} (capped at n and at rmax), a 'u' block in the middle of the list"""
    blk, ranks = [], []
    for n in SIZES:
        for r in sorted({min(r, n, rmax) for r in (0, 1, 3, 4, 5, n)}):
            blk.append(n)
            ranks.append(r)
    half = len(blk) // 2
    return blk[:half] + [-5] + blk[half:], ranks[:half] + [0] + ranks[half:]


# rmax = 130: r = n on every size; rmax = 6 < n: the column stride is min(n, rmax) in the wavefront and the workgroup class; the large
# blocks (split over workgroups from 257 on) with rmax = 8 < n: n = 300 at r = rmax, n = 1100 at r = 4 < rmax, a small one beside them
CASES = {"full": (130, None), "strided": (6, None), "large": (8, ([300, -3, 1100, 17], [8, 0, 4, 6]))}


@pytest.mark.parametrize("exact", [False, True], ids=["contract", "integers"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_writes_every_slot_within_its_contract(name, exact):
    rmax, lst = CASES[name]
    blk, ranks = lst if lst else small_list(rmax)
    rng = np.random.default_rng(len(blk) + rmax)
    Ls = factors(blk, ranks, rng, exact)
    got = op(blk, Ls, rmax, prefilled(blk))
    check_blocks(blk, Ls, got, exact)
    assert same_bits(op(blk, Ls, rmax, prefilled(blk)), got)              # the same bits from run to run


def test_kernel_refuses_bad_ranks_before_the_device():
    lib = cuadmm_amd.load()
    blk = np.array([5, -2, 40], np.int32)
    d = Dev(np.full(15 + 2 + 820, 3.0))
    L = np.ones(lowrank_size(blk, 8))
    for ranks, rmax in (([6, 0, 1], 8), ([1, 0, 9], 8), ([-1, 0, 1], 8), ([1, 0, 1], 0), ([1, 0, 1], 8193)):
        assert lib.cuadmm_op_block_outer(P(L), P(np.array(ranks, np.int32)), P(blk), 3, rmax, d.ptr, None) == -1, (ranks, rmax)
    assert lib.cuadmm_op_block_outer(None, P(np.array([0, 0, 1], np.int32)), P(blk), 3, 8, d.ptr, None) == -1
    assert np.all(d.get() == 3.0)
    # every rank 0 needs no factor buffer
    assert lib.cuadmm_op_block_outer(None, P(np.array([0, 9, 0], np.int32)), P(blk), 3, 8, d.ptr, None) == 0
    v = d.get()
    assert same_bits(v[:15], np.zeros(15)) and np.all(v[15:17] == 3.0) and same_bits(v[17:], np.zeros(820))


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


def raw(s, which, L, ranks, rmax, sig=0.0, out=True):
    """(rc, out4) of cuadmm_set_lowrank"""
    o = np.full(4, np.nan) if out else None
    rc = cuadmm_amd.load().cuadmm_set_lowrank(s._h, which, P(L), P(ranks), rmax, sig, P(o))
    return rc, o


def fixture_factors(seed, ranks=(2, 5, 7, 0, 16)):
    return factors(BLK_A, ranks, np.random.default_rng(seed), False)


def psd_mask(blk):
    off = offsets(blk)
    m = np.zeros(int(off[-1]), bool)
    for k, n in enumerate(blk):
        m[off[k]:off[k + 1]] = n > 0
    return m


def _traj(s):
    return [s.info_arr(k).copy() for k in INFO] + [s.X, s.y, s.S]


@pytest.mark.parametrize("which", [0, 1])
def test_fresh_solver_gets_the_kernels_bits_and_nothing_else_changes(which):
    fx = fixture()
    s = solver(fx, fx.Xs, fx.ys, fx.Ss)
    X0, y0, S0 = s.X, s.y, s.S
    rmax = 20                                                               # < 70, 130: strided columns; ranks up to 16
    Ls = fixture_factors(3 + which)
    L, ranks = pack_nan(BLK_A, Ls, rmax)
    rc, o = raw(s, which, L, ranks, rmax)
    assert rc == 0, cuadmm_amd.load().cuadmm_last_error()
    before = (X0, S0)[which]
    want = op(BLK_A, Ls, rmax, before)                                      # the 'u' block keeps the bits it had
    got = (s.X, s.S)[which]
    psd = psd_mask(BLK_A)
    assert same_bits(got, want) and same_bits(got[~psd], before[~psd]) and not same_bits(got[psd], before[psd])
    assert same_bits(s.y, y0) and same_bits((s.S, s.X)[which], (S0, X0)[which])
    # out4: the counts passed in, the kernel's time, the factor buffer staged whole
    assert o[0] == 4 and o[1] == 2 + 5 + 7 + 16 and o[2] > 0 and o[3] == 8 * lowrank_size(BLK_A, rmax)
    # every rank 0 and no buffer: + 0.0 on every PSD block, nothing staged; out4 may be null
    rc, o = raw(s, which, None, np.zeros(5, np.int32), 1)
    z = (s.X, s.S)[which]
    assert rc == 0 and o[0] == 4 and o[1] == 0 and o[3] == 0 and same_bits(z[psd], np.zeros(int(psd.sum()))) and same_bits(z[~psd], before[~psd])
    assert raw(s, which, L, ranks, rmax, out=False)[0] == 0 and same_bits((s.X, s.S)[which], want)
    # sig > 0 sets sigma
    assert s.state()["sig"] == 1.0 and raw(s, which, L, ranks, rmax, sig=2.5)[0] == 0 and s.state()["sig"] == 2.5


@pytest.mark.parametrize("which", [0, 1])
def test_behind_a_solve_it_is_set_XyS_for_that_vector(which):
    """Three solvers after the same 30 iterations (the scaled state pending).  a: the getters, for what X, y, S are in the caller's units.
    b: set_lowrank straight onto the pending state.  c: set_XyS with the vector b then returns."""
    fx = fixture()
    a, b, c = (solver(fx) for _ in range(3))
    for s in (a, b, c):
        s.solve(30, 0.0)
    Xa, ya, Sa = a.X, a.y, a.S
    assert b.status()["status"] == 2
    Ls = fixture_factors(11 + which, ranks=(1, 4, 9, 0, 12))
    Lp, ranks, rmax = cuadmm_amd.solver.pack_lowrank(BLK_A, Ls)
    rc, o = raw(b, which, Lp, ranks, rmax)
    assert rc == 0 and o[1] == 26
    before = (Xa, Sa)[which]
    new = (b.X, b.S)[which]
    assert same_bits(new, op(BLK_A, Ls, rmax, before))
    assert same_bits(b.y, ya) and same_bits((b.S, b.X)[which], (Sa, Xa)[which])
    # status and gap information are reset as set_XyS resets them
    c.set_XyS(**{"XS"[which]: new})
    assert b.status()["status"] == 0 and b.status() == c.status() and b.gap_info() == c.gap_info()
    for s in (b, c):
        s.solve(5, 0.0, if_first=False)
    for u, v in zip(_traj(b), _traj(c)):
        assert same_bits(u, v)
    assert b.info_iter_num == 5


def test_round_trip_through_lowrank():
    fx = fixture()
    rng = np.random.default_rng(21)
    off = offsets(BLK_A)
    X = rng.standard_normal(int(off[-1]))
    for k, n in enumerate(BLK_A):
        if n > 0:
            G = rng.standard_normal((n, min(5, n)))
            ii, jj = np.tril_indices(n)
            M = G @ G.T
            X[off[k]:off[k + 1]] = np.where(ii == jj, M[ii, jj], M[ii, jj] * np.sqrt(2.0))
    s = solver(fx)
    s.set_XyS(X=X)
    old = s.X
    assert same_bits(old, X)
    f = s.lowrank("X", tol=1e-10)
    assert f["rank"].tolist() == [3, 5, 5, 0, 5]
    res = s.set_lowrank(X=f["L"])["X"]
    assert res["blocks"] == 4 and res["rank_sum"] == 18 and res["bytes_staged"] == 8 * lowrank_size(BLK_A, 5)
    new = s.X
    for k, n in enumerate(BLK_A):
        o, n_ = new[off[k]:off[k + 1]], old[off[k]:off[k + 1]]
        if n < 0:
            assert same_bits(o, n_)
            continue
        Lk = np.abs(f["L"][k].astype(LD))
        r = Lk.shape[1]
        diff = float(np.sqrt(np.sum((o.astype(LD) - n_.astype(LD)) ** 2)))          # ||.||_F of the block = 2-norm of its svec
        bound = f["resid"][k] + 4 * (n + 2) * U * f["trace"][k] + (r + 4) * U * np.sqrt(2.0) * float(np.sqrt(np.sum((Lk @ Lk.T) ** 2)))
        print("block", k, "n", n, "r", r, "||X_new - X_old||_F %.3e" % diff, "bound %.3e" % bound)
        assert diff <= bound, (k, diff, bound)
    assert s.lowrank("X", tol=1e-10)["rank"].tolist() == [3, 5, 5, 0, 5]


def test_refusals_leave_the_solver_as_it_was(tmp_path):
    fx = fixture()
    lib = cuadmm_amd.load()
    a, b = solver(fx), solver(fx)
    for s in (a, b):
        s.solve(20, 0.0)
    rmax = 16
    Ls = fixture_factors(31)
    L, ranks = pack_nan(BLK_A, Ls, rmax)
    loff = np.concatenate([[0], np.cumsum([n * min(n, rmax) if n > 0 else 0 for n in BLK_A])])

    def with_rank(k, r):
        q = ranks.copy()
        q[k] = r
        return q

    def with_entry(k, col, row, x):
        q = L.copy()
        q[loff[k] + col * BLK_A[k] + row] = x
        return q

    def refused(s):
        for args in ((-1, L, ranks, rmax), (2, L, ranks, rmax), (0, L, ranks, 0), (0, L, ranks, 8193), (0, L, None, rmax),
                     (0, L, with_rank(1, -1), rmax), (1, L, with_rank(2, 17), rmax), (0, L, with_rank(0, 4), rmax), (1, None, ranks, rmax),
                     (0, with_entry(2, 6, 69, np.nan), ranks, rmax), (1, with_entry(4, 0, 0, np.inf), ranks, rmax), (0, with_entry(1, 4, 19, -np.inf), ranks, rmax)):
            rc, o = raw(s, *args)
            assert rc == -1 and np.all(np.isnan(o)), args[0]                # CUADMM_ERR_INVALID, out4 untouched
            assert "set_lowrank" in lib.cuadmm_last_error().decode()
    # a NaN in a column that is not read is no reason to refuse (block 2 has 7 columns: column 7 is not one of them)
    assert np.isnan(L[loff[2] + 7 * 70])
    refused(a)                                                              # on the pending scaled state: it must stay pending
    for s in (a, b):
        s.solve(5, 0.0, if_first=False)
    refused(a)
    ta, tb = _traj(a), _traj(b)
    for u, v in zip(ta, tb):
        assert same_bits(u, v)
    refused(a)                                                              # in the caller's units now
    for u, v in zip((a.X, a.y, a.S), tb[-3:]):
        assert same_bits(u, v)
    # not initialised; more than one rank; the leader of an in-process group
    fresh = cuadmm_amd.SDPSolver(verbose=False)
    assert raw(fresh, 0, L, ranks, rmax)[0] == -1
    w = cuadmm_amd.SDPSolver(verbose=False, rank=0, world=2)
    w.set_allreduce(lambda ptr, count, stream: None)
    w.init_problem(amd(fx))
    assert raw(w, 0, L, ranks, rmax)[0] == -1 and "one rank" in lib.cuadmm_last_error().decode()
    blk_g = [6, 10, 6, 10]                                                  # (the duo front end takes two block sizes)
    p = amd(make_opt_fixture(blk_g, 8, 9))
    g = cuadmm_amd.SDPSolver(verbose=False, options={"duo_share_device": 1})
    g.duo_init(True, 2, 15, 30, p.vec_len, p.con_num, p.At_csc_col_ptrs, p.At_csc_row_ids, p.At_csc_vals, p.At_nnz, p.b_indices, p.b_vals, p.b_nnz,
               p.C_indices, p.C_vals, p.C_nnz, p.blk_vals, p.mat_num)
    assert g.group_info()["engines"] == 2
    Lg, rg, mg = cuadmm_amd.solver.pack_lowrank(blk_g, factors(blk_g, (2, 2, 2, 2), np.random.default_rng(5), False))
    Xg = g.X
    assert raw(g, 0, Lg, rg, mg)[0] == -1 and "one rank" in lib.cuadmm_last_error().decode() and same_bits(g.X, Xg)
    # the Python front end: a wrong row count, a wrong number of entries
    bad = [m.copy() for m in Ls]
    bad[1] = np.zeros((19, 2))
    for arg in (bad, Ls[:4]):
        with pytest.raises(ValueError):
            a.set_lowrank(X=arg)
    with pytest.raises(ValueError):
        a.set_lowrank(S=bad)
    for u, v in zip((a.X, a.y, a.S), tb[-3:]):
        assert same_bits(u, v)


# ---- 3. the front ends ----------------------------------------------------------------------------------------------------
FACADE = r'''
#include <cstdio>
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
    SDPSolver solver;
    solver.set_option("verbose", 0.0);
    solver.init(15, 30, problem.vec_len, problem.con_num, problem.At_csc_col_ptrs.data(), problem.At_csc_row_ids.data(), problem.At_csc_vals.data(),
                problem.At_nnz, problem.b_indices.data(), problem.b_vals.data(), problem.b_nnz, problem.C_indices.data(), problem.C_vals.data(),
                problem.C_nnz, blk_vals.data(), problem.mat_num, problem.X_vals.data(), problem.y_vals.data(), problem.S_vals.data(), 1.0);
    solver.solve(60, 0.0, false, 50, 100, 5000);
    const SDPSolver::LowRank r = solver.lowrank(0, 1e-10, 6);
    std::vector<int> ranks;
    for (size_t k = 0; k < r.per_block.size() / 6; ++k) ranks.push_back((int)r.per_block[6 * k]);
    const SDPSolver::LowRankStart st = solver.set_lowrank(0, r.L.data(), ranks.data(), 6);
    std::printf("START %d %.0f %.0f %.0f %d\n", st.blocks, st.rank_sum, r.rank_sum, st.bytes_staged, st.ms > 0 ? 1 : 0);
    solver.solve(5, 0.0, false, 50, 100, 5000, 1.05, false);
    std::printf("ITER %d\n", solver.info_iter_num);
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


def test_command_line_and_facade(tmp_path):
    fx = make_opt_fixture(BLK_C, M_C, 5)
    d, out = str(tmp_path / "prob") + "/", str(tmp_path / "factors") + "/"
    _write_txt(d, fx)
    os.makedirs(out)
    libdir = os.path.join(ROOT, "cuadmm_amd", "lib")
    exe = os.path.join(libdir, "cuadmm_exe")
    lib = cuadmm_amd.load()
    # run 1 writes the factors; y beside them as the program writes vectors
    r = subprocess.run([exe, d, "--lowrank=1e-10", "--lowrank-out=" + out, "--max_iter=80", "--stop_tol=0", "--quiet"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    y0 = 0.5 * fx.ys
    assert lib.cuadmm_write_dense_txt((out + "y.txt").encode(), P(y0), y0.size) == 0
    # run 2 starts from them
    js = str(tmp_path / "b.json")
    r = subprocess.run([exe, d, "--start-lowrank=" + out, "--max_iter=5", "--stop_tol=0", "--quiet", "--json=" + js], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count(" start(") == 2 and " start(X): 3 blocks from factors, rank sum " in r.stdout
    with open(js) as f:
        side = json.load(f)
    # the binding from the same files
    numbers = lambda fn: np.array(open(fn).read().split(), np.float64)        # (a block of rank 0 has an empty file)
    Ls = {w: [numbers(out + "L_%s_%d.txt" % (w, k)).reshape(-1, n).T if n > 0 else np.zeros((0, 0)) for k, n in enumerate(BLK_C)] for w in "XS"}
    prob = cuadmm_amd.Problem.from_txt(d)
    s = cuadmm_amd.SDPSolver(verbose=False, profile=True)
    s.init_problem(prob)
    got = s.set_lowrank(X=Ls["X"], S=Ls["S"])
    s.set_XyS(y=np.loadtxt(out + "y.txt"))
    s.solve(5, 0.0, 0, 50, 100, 5000, 1.05, if_first=False)
    st = s.state()
    assert side["iterations"] == 5
    for key in ("pobj", "dobj", "errRp", "errRd"):
        assert side[key] == st[key], (key, side[key], st[key])
    assert side["start_lowrank"]["y"] is True
    for w in "XS":
        assert side["start_lowrank"][w]["rank_sum"] == got[w]["rank_sum"] == sum(m.shape[1] for m in Ls[w]) > 0
        assert side["start_lowrank"][w]["blocks"] == 3 and side["start_lowrank"][w]["bytes_staged"] == got[w]["bytes_staged"]
    # a factor file with n_k r_k + 1 numbers: exit code 1 and a message, no solve
    bad = out + "L_S_1.txt"
    with open(bad, "a") as f:
        f.write("1.0\n")
    os.remove(d + "X_opt.txt")
    r = subprocess.run([exe, d, "--start-lowrank=" + out, "--max_iter=5", "--quiet"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--start-lowrank" in r.stderr and "L_S_1.txt" in r.stderr and "multiple of 12" in r.stderr
    assert " start(" not in r.stdout and not os.path.exists(d + "X_opt.txt")
    with open(bad, "w") as f:
        f.write("0.5\n" * (12 * 12 + 12))
    r = subprocess.run([exe, d, "--start-lowrank=" + out, "--max_iter=5", "--quiet"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "at most 144" in r.stderr and not os.path.exists(d + "X_opt.txt")
    # the C++ facade
    src, fexe = tmp_path / "facade.cpp", tmp_path / "facade"
    src.write_text(FACADE)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(fexe), "-L" + libdir,
                           "-lcuadmm_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([str(fexe), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("START ")][0]
    assert int(line[1]) == 3 and line[2] == line[3] and int(line[4]) == 8 * lowrank_size(BLK_C, 6) and line[5] == "1"
    assert "ITER 5" in r.stdout
