"""Op-level tests of the kernels an ADMM iteration launches (csrc/vec_kernels.hip), through the test hooks cuadmm_op_aty_xb, _post,
_spmv_rows, _forest_solve and _rp_stats.  References: the same expressions in np.longdouble.  Bounds are derived, not measured, and
asserted PER ROW, so that one wrong short row cannot hide behind a long one:
  sparse dot product of n terms:  |got - ref| <= (n + 2) 2^-53 (sum |a_i x_i| + |c|)      (any summation order, with or without FMA)
  elementwise update:             2 ulp of the largest term, plus what the inputs' own bounds carry through
  the two sums over N elements:   (N + 2) 2^-53 sum |terms|, plus the terms' own bounds
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import cuadmm_amd
from cuadmm_amd._lib import check
from tests import helpers as H

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
F64 = lambda a: np.asarray(a, dtype=np.float64)


def csr_from_lengths(lengths, ncols, rng):
    lengths = np.asarray(lengths, dtype=np.int64)
    rp = np.zeros(lengths.size + 1, np.int32)
    rp[1:] = np.cumsum(lengths)
    nnz = int(rp[-1])
    ci = rng.integers(0, ncols, nnz).astype(np.int32)
    av = rng.standard_normal(nnz)
    return rp, ci, av


def row_sums(rp, vals):
    """per-row sums of `vals` (any dtype) over a CSR row pointer; empty rows give 0"""
    out = np.zeros(rp.size - 1, vals.dtype)
    ne = rp[1:] > rp[:-1]
    if vals.size:
        out[ne] = np.add.reduceat(vals, rp[:-1][ne].astype(np.int64))
    return out


# ---------------------------------------------------------------------------------------------------------------- aty_xb
def aty_gpu(rp, ci, av, y, Cv, X, sig, write_xb, Rd1_in=None, Xb_in=None):
    lib = cuadmm_amd.load()
    L = rp.size - 1
    Rd1 = np.full(L, np.nan) if Rd1_in is None else Rd1_in.copy()
    Xb = np.full(L, np.nan) if Xb_in is None else Xb_in.copy()
    info = np.zeros(2, np.int32)
    check(lib.cuadmm_op_aty_xb(L, y.size, P(rp), P(ci), P(av), P(y), P(Cv), P(X), float(sig), int(write_xb), P(Rd1), P(Xb), P(info)))
    return Rd1, Xb, int(info[0]), int(info[1])


def aty_check(rp, ci, av, y, Cv, X, sig, Rd1, Xb):
    n = (rp[1:] - rp[:-1]).astype(np.float64)
    prod = av.astype(LD) * y[ci].astype(LD)
    ref = row_sums(rp, prod) - Cv.astype(LD)
    mag = F64(row_sums(rp, np.abs(prod))) + np.abs(Cv)
    tol = (n + 2) * U * mag
    bad = np.nonzero(~(np.abs(F64(Rd1.astype(LD) - ref)) <= tol))[0]
    assert bad.size == 0, "Rd1 rows %s (lengths %s)" % (bad[:8], n[bad[:8]])
    if Xb is not None:
        refx = X.astype(LD) + LD(sig) * ref
        tolx = abs(sig) * tol + 4 * U * np.maximum(np.abs(X), np.abs(sig * F64(ref)))
        bad = np.nonzero(~(np.abs(F64(Xb.astype(LD) - refx)) <= tolx))[0]
        assert bad.size == 0, "Xb rows %s" % bad[:8]


def aty_problem(lengths, m, seed):
    rng = np.random.default_rng(seed)
    rp, ci, av = csr_from_lengths(lengths, m, rng)
    L = rp.size - 1
    return rp, ci, av, rng.standard_normal(m), rng.standard_normal(L), rng.standard_normal(L)


PASS = 4 * 4096 * 256        # rows one pass of the four-rows-per-thread grid covers once its grid is at its cap


@pytest.mark.parametrize("L", [1, 3, 4, 5, 1023, 1024, 1025, PASS - 1, PASS, PASS + 1, 2 * PASS - 1, 2 * PASS, 2 * PASS + 1])
def test_aty_xb_plain_kernel_sizes(L):
    rng = np.random.default_rng(L)
    lengths = rng.integers(0, 4, L) * (rng.random(L) < (0.9 if L < 5000 else 0.12))     # many empty rows
    if L >= 4:
        lengths[[0, L - 1]] = (24, 3)
    rp, ci, av, y, Cv, X = aty_problem(lengths, 777, L + 1)
    Rd1, Xb, nlong, max_short = aty_gpu(rp, ci, av, y, Cv, X, 1.7, 1)
    assert nlong == 0 and max_short <= 24                              # one thread per row
    aty_check(rp, ci, av, y, Cv, X, 1.7, Rd1, Xb)


@pytest.mark.parametrize("longest,g8", [(24, False), (25, True)])
def test_aty_xb_eight_lanes_per_row_from_25_entries(longest, g8):
    rng = np.random.default_rng(longest)
    L = 3001
    lengths = rng.integers(0, longest + 1, L)
    lengths[[0, 7, L - 1]] = longest
    lengths[[1, 8, L - 2]] = 0
    rp, ci, av, y, Cv, X = aty_problem(lengths, 500, 5)
    Rd1, Xb, nlong, max_short = aty_gpu(rp, ci, av, y, Cv, X, 0.3, 1)
    assert nlong == 0 and max_short == longest and (max_short > 24) == g8
    aty_check(rp, ci, av, y, Cv, X, 0.3, Rd1, Xb)


@pytest.mark.parametrize("longest,nlong_want", [(128, 0), (129, 2)])
def test_aty_xb_rows_of_128_stay_short_129_go_to_the_long_list(longest, nlong_want):
    rng = np.random.default_rng(longest)
    L = 2050
    lengths = rng.integers(0, 100, L)
    lengths[[3, L - 1]] = longest
    lengths[[4, 5]] = (127, 128)
    rp, ci, av, y, Cv, X = aty_problem(lengths, 900, 6)
    Rd1, Xb, nlong, max_short = aty_gpu(rp, ci, av, y, Cv, X, 2.5, 1)
    assert nlong == nlong_want and max_short == 128
    aty_check(rp, ci, av, y, Cv, X, 2.5, Rd1, Xb)


def test_aty_xb_long_rows_beside_g8_rows_canary_and_determinism():
    rng = np.random.default_rng(9)
    L = 5003
    lengths = rng.integers(0, 6, L)
    lengths[[0, 17, 2500, L - 1]] = (2720, 100000, 2720, 100000)
    lengths[[1, 18, 2501, L - 2]] = (60, 128, 25, 0)
    rp, ci, av, y, Cv, X = aty_problem(lengths, 120000, 10)
    Rd1, Xb, nlong, max_short = aty_gpu(rp, ci, av, y, Cv, X, 0.9, 1)
    assert nlong == 4 and max_short == 128
    aty_check(rp, ci, av, y, Cv, X, 0.9, Rd1, Xb)
    Rd1b, Xbb, _, _ = aty_gpu(rp, ci, av, y, Cv, X, 0.9, 1)
    assert np.array_equal(Rd1, Rd1b) and np.array_equal(Xb, Xbb)      # fixed summation orders: the same bits
    # write_xb = 0: Rd1 as before, a NaN-filled Xb untouched bit for bit
    canary = np.frombuffer(np.full(L, 0x7ff8000000c0ffee, np.uint64).tobytes(), np.float64)
    Rd1c, Xbc, _, _ = aty_gpu(rp, ci, av, y, Cv, X, 0.9, 0, Xb_in=canary)
    assert np.array_equal(Rd1c, Rd1)
    assert np.array_equal(Xbc.view(np.uint64), canary.view(np.uint64))
    # the same without long rows: the plain and the eight-lane kernels' own WRITE_XB = false variants
    for longest in (20, 40):
        rp2, ci2, av2, y2, C2, X2 = aty_problem(rng.integers(0, longest + 1, 1500), 300, longest)
        r, xb, _, ms = aty_gpu(rp2, ci2, av2, y2, C2, X2, 0.9, 0, Xb_in=canary[:1500])
        assert (ms > 24) == (longest == 40)
        aty_check(rp2, ci2, av2, y2, C2, X2, 0.9, r, None)
        assert np.array_equal(xb.view(np.uint64), canary[:1500].view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------ post
def post_gpu(mode, Xp, Rd1, Cv, X, S, inv_sig, tau_sig, sums, aty=None):
    lib = cuadmm_amd.load()
    L = Cv.size
    X, S, sums = X.copy(), S.copy(), sums.copy()
    nparts = C.c_int(-1)
    if aty is None:
        check(lib.cuadmm_op_post(mode, L, P(Xp), P(Rd1), P(Cv), P(X), P(S), float(inv_sig), float(tau_sig), P(sums), 0, None, None, None, None, C.byref(nparts)))
    else:
        rp, ci, av, y = aty
        check(lib.cuadmm_op_post(3, L, None, None, P(Cv), P(X), P(S), float(inv_sig), float(tau_sig), P(sums), y.size, P(rp), P(ci), P(av), P(y), C.byref(nparts)))
    return X, S, sums, nparts.value


def post_check_x_and_sums(r1, tol_r1, s, tol_s, X0, Cv, tau_sig, X, sums):
    """r1, s: longdouble references with their float64 bounds; checks X (per element) and the two sums"""
    rd = r1 + s
    tol_rd = tol_r1 + tol_s + 4 * U * np.maximum(np.abs(F64(r1)), np.abs(F64(s)))
    xn = X0.astype(LD) + LD(tau_sig) * rd
    tol_x = abs(tau_sig) * tol_rd + 4 * U * np.maximum(np.abs(X0), np.abs(tau_sig * F64(rd)))
    bad = np.nonzero(~(np.abs(F64(X.astype(LD) - xn)) <= tol_x))[0]
    assert bad.size == 0, "X elements %s" % bad[:8]
    N = X0.size
    rdf = np.abs(F64(rd))
    t0 = (N + 2) * U * float(np.sum(rdf * rdf)) + float(np.sum(2 * rdf * tol_rd + tol_rd * tol_rd + 2 * U * rdf * rdf))
    t1 = (N + 2) * U * float(np.sum(np.abs(Cv * F64(xn)))) + float(np.sum(np.abs(Cv) * tol_x + 2 * U * np.abs(Cv * F64(xn))))
    assert abs(float(LD(sums[0]) - np.sum(rd * rd))) <= t0
    assert abs(float(LD(sums[1]) - np.sum(Cv.astype(LD) * xn))) <= t1


def bits(a):
    return a.view(np.uint64)


# L -> pairs the final reduction sees (post_grid: one workgroup per 1 024 elements, at most 2 048)
@pytest.mark.parametrize("L,nparts_want", [(1, 1), (1000, 1), (255 * 1024, 255), (255 * 1024 + 1, 256), (256 * 1024 + 1, 257), (2048 * 1024 + 77, 2048)])
def test_post_modes_and_the_pair_reduction(L, nparts_want):
    rng = np.random.default_rng(L)
    Xp, Rd1, Cv, X0, S0 = (rng.standard_normal(L) for _ in range(5))
    inv_sig, tau_sig = 1 / 1.3, 1.618 * 1.3
    canary = np.frombuffer(np.array([0x7ff8000000c0ffee, 0x7ff8000000c0ffef], np.uint64).tobytes(), np.float64)
    s_ref = LD(inv_sig) * (Xp.astype(LD) - X0.astype(LD)) - Rd1.astype(LD)
    tol_s = 4 * U * np.maximum(np.abs(inv_sig * (Xp - X0)), np.abs(Rd1)) + abs(inv_sig) * 2 * U * np.maximum(np.abs(Xp), np.abs(X0))
    zero = np.zeros(L)
    # mode 0: S, X, sums
    X, S, sums, nparts = post_gpu(0, Xp, Rd1, Cv, X0, S0, inv_sig, tau_sig, canary)
    assert nparts == nparts_want
    bad = np.nonzero(~(np.abs(F64(S.astype(LD) - s_ref)) <= tol_s))[0]
    assert bad.size == 0, "S elements %s" % bad[:8]
    post_check_x_and_sums(Rd1.astype(LD), zero, s_ref, tol_s, X0, Cv, tau_sig, X, sums)
    X_again, S_again, sums_again, _ = post_gpu(0, Xp, Rd1, Cv, X0, S0, inv_sig, tau_sig, canary)
    assert np.array_equal(X, X_again) and np.array_equal(S, S_again) and np.array_equal(sums, sums_again)
    # mode 1: S only -- X and the sums keep their bits
    X1, S1, sums1, _ = post_gpu(1, Xp, Rd1, Cv, X0, S0, inv_sig, tau_sig, canary)
    assert np.array_equal(bits(S1), bits(S))
    assert np.array_equal(bits(X1), bits(X0)) and np.array_equal(bits(sums1), bits(canary))
    # mode 2: X and sums from the S given -- S keeps its bits
    Snan = S0.copy()
    X2, S2, sums2, _ = post_gpu(2, Xp, Rd1, Cv, X0, Snan, inv_sig, tau_sig, canary)
    assert np.array_equal(bits(S2), bits(Snan))
    post_check_x_and_sums(Rd1.astype(LD), zero, S0.astype(LD), zero, X0, Cv, tau_sig, X2, sums2)


@pytest.mark.parametrize("L", [1, 1025, 300001])
def test_post_one_pass_second_half_matches_aty_then_mode_2(L):
    rng = np.random.default_rng(L + 5)
    rp, ci, av, y, Cv, X0 = aty_problem(rng.integers(0, 20, L), 400, L)
    S0 = rng.standard_normal(L)
    tau_sig = 2.1
    sums_in = np.zeros(2)
    X3, S3, sums3, nparts = post_gpu(3, None, None, Cv, X0, S0, 0.0, tau_sig, sums_in, aty=(rp, ci, av, y))
    assert nparts == min(2048, (L + 1023) // 1024)
    assert np.array_equal(bits(S3), bits(S0))
    n = (rp[1:] - rp[:-1]).astype(np.float64)
    prod = av.astype(LD) * y[ci].astype(LD)
    r1 = row_sums(rp, prod) - Cv.astype(LD)
    tol_r1 = (n + 2) * U * (F64(row_sums(rp, np.abs(prod))) + np.abs(Cv))
    post_check_x_and_sums(r1, tol_r1, S0.astype(LD), np.zeros(L), X0, Cv, tau_sig, X3, sums3)
    # the two-launch sequence it replaced
    Rd1, _, _, _ = aty_gpu(rp, ci, av, y, Cv, X0, 1.0, 0)
    X2, _, sums2, _ = post_gpu(2, np.zeros(L), Rd1, Cv, X0, S0, 0.0, tau_sig, sums_in)
    post_check_x_and_sums(r1, tol_r1, S0.astype(LD), np.zeros(L), X0, Cv, tau_sig, X2, sums2)
    assert np.array_equal(X2, X3) and np.array_equal(sums2, sums3)     # "same expressions" (vec_kernels.hip, aty_post2_kernel)


# -------------------------------------------------------------------------------------------------------------- spmv_rows
def spmv_gpu(rp, ci, av, X, S, Cv, want_x, want_s, rowmap=None, out_len=None):
    lib = cuadmm_amd.load()
    rows = rp.size - 1
    out_len = rows if out_len is None else out_len
    canary = np.frombuffer(np.full(out_len, 0x7ff8000000c0ffee, np.uint64).tobytes(), np.float64)
    oX, oS = canary.copy(), canary.copy()
    info = np.zeros(4, np.int32)
    check(lib.cuadmm_op_spmv_rows(rows, X.size, P(rp), P(ci), P(av), P(X), P(S), P(Cv), int(want_x), int(want_s), P(rowmap), out_len, P(oX), P(oS), P(info)))
    return oX, oS, dict(T=int(info[0]), cap=int(info[1]), nlong=int(info[2]), nseg=int(info[3])), canary


def spmv_check(rp, ci, av, X, S, Cv, oX, oS, slots=None):
    n = (rp[1:] - rp[:-1]).astype(np.float64)
    slots = np.arange(rp.size - 1) if slots is None else slots
    if oX is not None:
        prod = av.astype(LD) * X[ci].astype(LD)
        tol = (n + 2) * U * F64(row_sums(rp, np.abs(prod)))
        bad = np.nonzero(~(np.abs(F64(oX[slots].astype(LD) - row_sums(rp, prod))) <= tol))[0]
        assert bad.size == 0, "A X rows %s (lengths %s)" % (bad[:8], n[bad[:8]])
    if oS is not None:
        prod = av.astype(LD) * (S[ci].astype(LD) - Cv[ci].astype(LD))
        tol = (n + 3) * U * F64(row_sums(rp, np.abs(av) * (np.abs(S[ci]) + np.abs(Cv[ci]))))
        bad = np.nonzero(~(np.abs(F64(oS[slots].astype(LD) - row_sums(rp, prod))) <= tol))[0]
        assert bad.size == 0, "A (S - C) rows %s (lengths %s)" % (bad[:8], n[bad[:8]])


@pytest.mark.parametrize("T,lo,hi", [(1, 0, 2), (2, 0, 3), (4, 0, 7), (8, 0, 13), (16, 3, 25), (32, 0, 55), (64, 0, 120)])
def test_spmv_rows_lanes_per_row(T, lo, hi):
    rng = np.random.default_rng(T)
    rows, ncols = 1237, 3000
    lengths = rng.integers(lo, hi + 1, rows)
    if T == 1:
        lengths = (rng.random(rows) < 0.8).astype(np.int64)
    lengths[[0, 5, rows - 1]] = (0, hi, hi - 1 if hi > 1 else 0)        # an empty row, rows that are no multiple of T
    rp, ci, av = csr_from_lengths(lengths, ncols, rng)
    X, S, Cv = (rng.standard_normal(ncols) for _ in range(3))
    oX, oS, info, canary = spmv_gpu(rp, ci, av, X, S, Cv, 1, 1)
    assert info["T"] == T and info["nlong"] == 0 and info["nseg"] == 0
    spmv_check(rp, ci, av, X, S, Cv, oX, oS)
    oX1, oS1, _, _ = spmv_gpu(rp, ci, av, X, S, Cv, 1, 0)
    assert np.array_equal(oX1, oX) and np.array_equal(bits(oS1), bits(canary))        # only A X
    oX2, oS2, _, _ = spmv_gpu(rp, ci, av, X, S, Cv, 0, 1)
    assert np.array_equal(oS2, oS) and np.array_equal(bits(oX2), bits(canary))        # only A (S - C)


def test_spmv_rows_long_rows_in_segments():
    rng = np.random.default_rng(21)
    rows, ncols, cap = 20000, 400000, 256
    lengths = rng.integers(0, 7, rows)
    where = [0, 11, 7000, 7001, 13000, rows - 1]
    lengths[where] = (cap, cap + 1, cap + 4096, cap + 4097, 320000, cap + 1)
    rp, ci, av = csr_from_lengths(lengths, ncols, rng)
    X, S, Cv = (rng.standard_normal(ncols) for _ in range(3))
    nseg = sum(-(-(int(n) - cap) // 4096) for n in lengths[where] if n > cap)
    oX, oS, info, canary = spmv_gpu(rp, ci, av, X, S, Cv, 1, 1)
    assert info == dict(T=4, cap=cap, nlong=5, nseg=nseg) and nseg == 1 + 1 + 2 + 79 + 1
    spmv_check(rp, ci, av, X, S, Cv, oX, oS)
    oXb, oSb, _, _ = spmv_gpu(rp, ci, av, X, S, Cv, 1, 1)
    assert np.array_equal(oX, oXb) and np.array_equal(oS, oSb)         # segments added in segment order: the same bits
    oX1, oS1, _, _ = spmv_gpu(rp, ci, av, X, S, Cv, 1, 0)
    assert np.array_equal(oX1, oX) and np.array_equal(bits(oS1), bits(canary))
    oX2, oS2, _, _ = spmv_gpu(rp, ci, av, X, S, Cv, 0, 1)
    assert np.array_equal(oS2, oS) and np.array_equal(bits(oX2), bits(canary))


def test_spmv_rows_compact_list_writes_exactly_the_mapped_slots():
    rng = np.random.default_rng(22)
    rows, ncols, out_len = 501, 2000, 3000
    rp, ci, av = csr_from_lengths(rng.integers(0, 12, rows), ncols, rng)
    X, S, Cv = (rng.standard_normal(ncols) for _ in range(3))
    rowmap = np.sort(rng.choice(out_len, rows, replace=False)).astype(np.int32)
    rowmap[[0, rows - 1]] = rowmap[[rows - 1, 0]]
    oX, oS, info, canary = spmv_gpu(rp, ci, av, X, S, Cv, 1, 1, rowmap=rowmap, out_len=out_len)
    assert info["T"] == 8 and info["nlong"] == 0
    spmv_check(rp, ci, av, X, S, Cv, oX, oS, slots=rowmap)
    rest = np.setdiff1d(np.arange(out_len), rowmap)
    assert np.array_equal(bits(oX[rest]), bits(canary[rest])) and np.array_equal(bits(oS[rest]), bits(canary[rest]))


# ----------------------------------------------------------------------------------------------------------- forest_solve
def test_forest_solve_one_thread_per_tree():
    lib = cuadmm_amd.load()
    A, k, _ = H.lead_case("forest")
    f = H.Factor(A, 0)
    try:
        m = f.m
        ax, asmc, b = (v[0] for v in H.lead_vectors(m, 3))
        isig = 0.7
        y = np.full(m, np.nan)
        info = np.zeros(2, np.int32)
        check(lib.cuadmm_op_forest_solve(f.h, m, P(ax), P(asmc), P(b), isig, P(y), P(info)))
        assert info[0] == 400 and info[1] == 64 and info[0] >= 256          # what the engine asks of a forest before it takes this kernel
        xr = f.solve_ref(H.lead_rhs(ax, asmc, b, isig), LD)
        rhs64 = -asmc + isig * (-ax + b)
        x64 = f.solve_ref(rhs64, np.float64)
        nrm = np.linalg.norm(F64(xr))
        e64 = np.linalg.norm(F64(x64 - xr)) / nrm
        err = np.linalg.norm(F64(y - xr)) / nrm
        print("LEADCASE %-26s trees=%d e64 %.2e err %.2e ratio %.2f" % ("forest (one thread/tree)", info[0], e64, err, err / max(e64, 2.0 ** -52)))
        assert e64 <= 1e-13 and err <= 8 * max(e64, 2.0 ** -52)           # MARGIN of tests/test_gpu_lead_solve.py
        host = np.empty(m)
        check(lib.cuadmm_aat_solve_permuted(f.h, P(rhs64), P(host)))
        assert np.array_equal(y, host)                                      # the serial host algorithm, unfused: bit for bit
    finally:
        f.close()


# --------------------------------------------------------------------------------------------------------------- rp_stats
@pytest.mark.parametrize("m", [1, 127, 128, 129, 100000])
def test_rp_stats(m):
    lib = cuadmm_amd.load()
    rng = np.random.default_rng(m)
    ax, b, y = (rng.standard_normal(m) for _ in range(3))
    normA = 1.0 + rng.random(m)
    bscale = 3.7
    sums = np.array([0.123, -4.5])
    out = np.full(4, np.nan)
    check(lib.cuadmm_op_rp_stats(m, P(ax), P(b), P(normA), P(y), bscale, P(sums), P(out)))
    ro = normA.astype(LD) * (b.astype(LD) - ax.astype(LD)) * LD(bscale)
    by = b.astype(LD) * y.astype(LD)
    # per term at most 8 roundings (three in ro, squared), then any summation order over m terms
    assert abs(float(LD(out[0]) - np.sum(ro * ro))) <= (m + 10) * U * float(np.sum(ro * ro))
    assert abs(float(LD(out[1]) - np.sum(by))) <= (m + 10) * U * float(np.sum(np.abs(by)))
    assert out[2] == sums[0] and out[3] == sums[1]
    out2 = np.full(4, np.nan)
    check(lib.cuadmm_op_rp_stats(m, P(ax), P(b), P(normA), P(y), bscale, P(sums), P(out2)))
    assert np.array_equal(out, out2)
