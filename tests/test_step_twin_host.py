"""tests/_step_twin.py without a device: its references at tiny sizes against plain Python loops (fractions.Fraction, math.fsum), its
checkers on what a plain float64 loop gives (accepted), and on that result with one thing wrong (refused, every time).
"""
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

from tests import _step_twin as T

U = T.U


def tiny_problem(seed=1, L=23, m=7):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 4, L)
    lengths[[2, 9]] = 0
    lengths[5] = 11
    rp = np.zeros(L + 1, np.int32)
    rp[1:] = np.cumsum(lengths)
    ci = rng.integers(0, m, rp[-1]).astype(np.int32)
    av, y = rng.standard_normal(rp[-1]), rng.standard_normal(m)
    Cv, X = rng.standard_normal(L), rng.standard_normal(L)
    idx = rng.permutation(L)[:12].astype(np.int32)
    idx[:2] = (2, 5)                                           # an empty row and the long one are listed
    idx = np.unique(idx)[::-1].copy()
    return rp, ci, av, y, Cv, X, idx


def loop_aty(rp, ci, av, y, Cv, X, sig, idx, Rd1_in, Xb_in):
    Rd1, Xb = Rd1_in.copy(), Xb_in.copy()
    for i in idx:
        t = 0.0
        for p in range(rp[i], rp[i + 1]):
            t += av[p] * y[ci[p]]
        Rd1[i] = t - Cv[i]
        Xb[i] = X[i] + Rd1[i] * sig
    return Rd1, Xb


def test_aty_reference_is_the_exact_row_sum_and_the_checker_takes_a_float_loop():
    rp, ci, av, y, Cv, X, idx = tiny_problem()
    sig = 1.7
    r, tol_r, xb, tol_xb = T.aty_xb_ref(rp, ci, av, y, Cv, X, sig)
    for i in range(rp.size - 1):
        exact = sum((Fr(av[p]) * Fr(y[ci[p]]) for p in range(rp[i], rp[i + 1])), Fr(0)) - Fr(Cv[i])
        mag = sum(abs(av[p] * y[ci[p]]) for p in range(rp[i], rp[i + 1])) + abs(Cv[i])
        assert abs(Fr(float(r[i])) - exact) <= Fr(2.0 ** -52) * Fr(abs(float(r[i]))) + Fr(2.0 ** -60) * Fr(mag)      # longdouble, read as float64
        assert tol_r[i] == (rp[i + 1] - rp[i] + 2) * U * mag or abs(tol_r[i] - (rp[i + 1] - rp[i] + 2) * U * mag) <= 4 * U * tol_r[i]
        assert abs(Fr(float(xb[i])) - (Fr(X[i]) + Fr(sig) * exact)) <= Fr(tol_xb[i]) + Fr(2.0 ** -52) * Fr(abs(float(xb[i])))
    L = rp.size - 1
    Rd1_in, Xb_in = np.arange(L) + 0.25, -np.arange(L) - 0.75
    Rd1, Xb = loop_aty(rp, ci, av, y, Cv, X, sig, idx, Rd1_in, Xb_in)
    T.check_aty_xb_idx(rp, ci, av, y, Cv, X, sig, idx, Rd1_in, Xb_in, Rd1, Xb)
    # one listed row skipped
    for arr_name in ("Rd1", "Xb"):
        bad = {"Rd1": Rd1.copy(), "Xb": Xb.copy()}
        bad[arr_name][idx[3]] = {"Rd1": Rd1_in, "Xb": Xb_in}[arr_name][idx[3]]
        with pytest.raises(AssertionError):
            T.check_aty_xb_idx(rp, ci, av, y, Cv, X, sig, idx, Rd1_in, Xb_in, bad["Rd1"], bad["Xb"])
    # one unlisted row written (with the value the kernel would give it)
    j = int(np.nonzero(T.unlisted(L, idx))[0][1])
    full = loop_aty(rp, ci, av, y, Cv, X, sig, np.arange(L), Rd1_in, Xb_in)
    for w in (0, 1):
        bad = [Rd1.copy(), Xb.copy()]
        bad[w][j] = full[w][j]
        with pytest.raises(AssertionError):
            T.check_aty_xb_idx(rp, ci, av, y, Cv, X, sig, idx, Rd1_in, Xb_in, bad[0], bad[1])
    # an empty listed row that is not exactly -C
    bad = Rd1.copy()
    bad[2] = np.nextafter(bad[2], np.inf)
    with pytest.raises(AssertionError):
        T.check_aty_xb_idx(rp, ci, av, y, Cv, X, sig, idx, Rd1_in, Xb_in, bad, Xb)


def loop_post_rest(mode, idx, fused, Xp, Rd1, Cv, X0, S0, inv_sig, tau_sig, use_quads, sums_in):
    X, S, sums = X0.copy(), S0.copy(), sums_in.copy()
    nfused, grid = fused.size // 2, (T.post_grid(idx.size) if idx.size else 0)
    part = np.concatenate([fused, np.full(2 * grid, np.nan)])
    acc = [[0.0, 0.0] for _ in range(grid)]
    for k, i in enumerate(idx):
        s = inv_sig * (Xp[i] - X0[i]) - Rd1[i]
        S[i] = s
        if mode == 0:
            rd = Rd1[i] + s
            X[i] = X0[i] + tau_sig * rd
            acc[(k // 256) % grid][0] += rd * rd
            acc[(k // 256) % grid][1] += Cv[i] * X[i]
    if mode == 0:
        for g in range(grid):
            part[2 * (nfused + g):2 * (nfused + g) + 2] = acc[g]
        if not use_quads:
            sums[:] = (sum(part[0::2]), sum(part[1::2]))
    return X, S, sums, part, (nfused + grid if use_quads else -1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("use_quads", [0, 1])
def test_post_rest_reference_and_checker(mode, use_quads):
    rng = np.random.default_rng(5)
    L = 1500
    Xp, Rd1, Cv, X0, S0 = (rng.standard_normal(L) for _ in range(5))
    idx = rng.permutation(L)[:1100].astype(np.int32)                        # two workgroups' worth
    fused = np.array([3.5, -1.25, 0.75, 2.0, 1e-3, -4.0])
    inv_sig, tau_sig = 1 / 1.3, 1.618 * 1.3
    sums_in = np.array([-7.0, 9.0])
    ref = T.post_rest_ref(idx, Xp, Rd1, Cv, X0, inv_sig, tau_sig)
    for k in (0, 17, 1099):
        i = idx[k]
        s = Fr(inv_sig) * (Fr(Xp[i]) - Fr(X0[i])) - Fr(Rd1[i])
        xn = Fr(X0[i]) + Fr(tau_sig) * (Fr(Rd1[i]) + s)
        assert abs(Fr(float(ref["s"][k])) - s) <= Fr(2.0 ** -52) * abs(s)
        assert abs(Fr(float(ref["xn"][k])) - xn) <= Fr(2.0 ** -52) * abs(xn)
        assert abs(Fr(float(ref["cx"][k])) - Fr(Cv[i]) * xn) <= Fr(2.0 ** -52) * abs(Fr(Cv[i]) * xn)
    args = (mode, idx, fused, Xp, Rd1, Cv, X0, S0, inv_sig, tau_sig, use_quads, sums_in)
    X, S, sums, part, nparts = loop_post_rest(*args)
    assert part.size == 2 * (3 + 2)
    T.check_post_rest(*args, X, S, sums, part, nparts)

    def refused(X=X, S=S, sums=sums, part=part, nparts=nparts):
        with pytest.raises(AssertionError):
            T.check_post_rest(*args, X, S, sums, part, nparts)

    # one element of an elementwise update 8 ulp off: the element whose bound is tightest against its own size
    k = int(np.argmax(np.abs(T.F64(ref["s"])) / ref["tol_s"]))
    off = S.copy()
    off[idx[k]] += 8 * np.spacing(abs(off[idx[k]]))
    assert 8 * np.spacing(abs(S[idx[k]])) > ref["tol_s"][k] + abs(float(S[idx[k]] - ref["s"][k]))      # (what makes this a test of the checker)
    refused(S=off)
    skipped = S.copy()
    skipped[idx[7]] = S0[idx[7]]
    refused(S=skipped)
    j = int(np.nonzero(T.unlisted(L, idx))[0][3])
    written = S.copy()
    written[j] = inv_sig * (Xp[j] - X0[j]) - Rd1[j]
    refused(S=written)
    refused(nparts=nparts + 1)
    moved = part.copy()
    moved[1] = np.nextafter(moved[1], 0)
    refused(part=moved)
    if mode == 0:
        k = int(np.argmax(np.abs(T.F64(ref["xn"])) / ref["tol_x"]))
        off = X.copy()
        off[idx[k]] += 8 * np.spacing(abs(off[idx[k]]))
        assert 8 * np.spacing(abs(X[idx[k]])) > ref["tol_x"][k] + abs(float(X[idx[k]] - ref["xn"][k]))
        refused(X=off)
        written = X.copy()
        written[j] += 1.0
        refused(X=written)
        short = part.copy()
        short[2 * 4:] = 0.0                                                 # the last workgroup's pair dropped
        refused(part=short)
        refused(sums=(sums_in + 1.0 if use_quads else np.array([sums[0] - float(ref["rd2"][5]), sums[1]])))
    else:
        touched = X.copy()
        touched[idx[0]] = np.nextafter(touched[idx[0]], np.inf)
        refused(X=touched)
        refused(sums=sums_in[::-1].copy())
        wrote = part.copy()
        wrote[-1] = 0.0
        refused(part=wrote)


def loop_quads(p1, p2):
    q1, q2 = p1.reshape(-1, 2), p2.reshape(-1, 2)
    return np.array([math.fsum(q2[:, 0]), math.fsum(q2[:, 1]), math.fsum(q1[:, 0]), math.fsum(q1[:, 1])])


def test_quad_sum_checkers_refuse_a_dropped_pair_a_doubled_pair_and_the_wrong_order():
    rng = np.random.default_rng(8)
    n1, n2 = 1300, 900
    for kind in ("int", "normal"):
        if kind == "int":
            p1, p2 = (rng.integers(-2 ** 20, 2 ** 20 + 1, 2 * n).astype(np.float64) for n in (n1, n2))
            assert T.quads_exact(p1, p2) == [int(math.fsum(p2[0::2])), int(math.fsum(p2[1::2])), int(math.fsum(p1[0::2])), int(math.fsum(p1[1::2]))]
            checks = (T.check_quads_exact, T.check_quads_bound)
        else:
            p1, p2 = rng.standard_normal(2 * n1), rng.standard_normal(2 * n2)
            checks = (T.check_quads_bound,)
        out4 = loop_quads(p1, p2)
        for chk in checks:
            chk(p1, p2, out4, out4[2:4].copy())
            # naive left-to-right float64 sums meet the bound as well
            chk(p1, p2, np.array([sum(p2[0::2]), sum(p2[1::2]), sum(p1[0::2]), sum(p1[1::2])]))
            for wrong in (loop_quads(p1[2:], p2),                                        # one pair dropped from p1
                          loop_quads(p1, np.delete(p2, [500, 501])),                     # ... from the middle of p2
                          loop_quads(np.concatenate([p1, p1[40:42]]), p2),               # one pair counted twice
                          loop_quads(p1, np.concatenate([p2, p2[-2:]])),
                          out4[[2, 3, 0, 1]]):                                           # [a, b, c, d] instead of [c, d, a, b]
                with pytest.raises(AssertionError):
                    chk(p1, p2, wrong)
            with pytest.raises(AssertionError):
                chk(p1, p2, out4, out4[[3, 2]].copy())
            with pytest.raises(AssertionError):
                chk(p1, p2, np.array([out4[0], np.nan, out4[2], out4[3]]))               # a read behind the pairs
    # batch: every iteration bit for bit, canary intact
    singles = [loop_quads(rng.standard_normal(10), rng.standard_normal(10)) for _ in range(3)]
    canary = np.array([1.5, -2.5, 3.5, np.nan])
    out = np.concatenate(singles + [canary])
    T.check_quads_batch(out, canary, singles)
    for at in (5, 12, 15):
        bad = out.copy()
        bad[at] = 0.0 if np.isnan(bad[at]) else np.nextafter(bad[at], np.inf)
        with pytest.raises(AssertionError):
            T.check_quads_batch(bad, canary, singles)
    assert [T.quad_segments(a, b) for a, b in ((0, 0), (1, 1), (16384, 16384), (16385, 1), (3, 32769))] == [1, 1, 1, 2, 3]
    assert [T.post_grid(n) for n in (1, 1024, 1025, 2048 * 1024 + 77)] == [1, 1, 2, 2048]


def test_closed_rows_reference_and_checker():
    rng = np.random.default_rng(4)
    nslots, m = 9, 40
    nk = np.array([1, 2, 3, 4, 5, 6, 7, 8, 3], np.int32)
    rows = np.stack([rng.permutation(m)[:8] for _ in range(nslots)]).astype(np.int32).reshape(-1)
    ax, as_, b = (rng.standard_normal(m) for _ in range(3))
    cl_in = np.arange(16 * nslots) + 0.5
    cl, bo = T.closed_rows_ref(nk, rows, ax, as_, b, cl_in)
    for s in range(nslots):
        for k in range(8):
            r = rows[8 * s + k]
            assert cl[16 * s + k] == (ax[r] if k < nk[s] else cl_in[16 * s + k])
            assert cl[16 * s + 8 + k] == (as_[r] if k < nk[s] else cl_in[16 * s + 8 + k])
            assert bo[8 * s + k].tobytes() == (b[r].tobytes() if k < nk[s] else bytes([0xA5] * 8))
    T.check_closed_rows(nk, rows, ax, as_, b, cl_in, cl, bo, 0)
    with pytest.raises(AssertionError):
        T.check_closed_rows(nk, rows, ax, as_, b, cl_in, cl, bo, 1)
    for arr, at in ((cl, 16 * 2 + 3), (cl, 16 * 2 + 8 + 2), (bo, 8 * 0 + 1), (bo, 8 * 7 + 7)):      # a slot past nk written, a slot below nk wrong
        bad = arr.copy()
        bad[at] = 0.0
        with pytest.raises(AssertionError):
            T.check_closed_rows(nk, rows, ax, as_, b, cl_in, bad if arr is cl else cl, bad if arr is bo else bo, 0)


def test_copy_checker_sees_one_missing_tail_byte_and_one_canary_byte():
    rng = np.random.default_rng(2)
    for nbytes in (4, 12, 20, 4096 + 12):
        src = rng.integers(1, 255, nbytes).astype(np.uint8)
        dst_in = np.full(nbytes + 32, 0xEE, np.uint8)
        out = dst_in.copy()
        out[:nbytes] = src
        T.check_copy(src, dst_in, out, nbytes)
        miss = out.copy()
        miss[nbytes - 1] = dst_in[nbytes - 1]                                  # one byte of the 4-byte tail missing
        with pytest.raises(AssertionError):
            T.check_copy(src, dst_in, miss, nbytes)
        over = out.copy()
        over[nbytes] = src[0]                                                  # one byte too many
        with pytest.raises(AssertionError):
            T.check_copy(src, dst_in, over, nbytes)
    src = rng.standard_normal(5)
    dst_in = np.concatenate([np.zeros(5), [np.nan, 1.0, 2.0, 3.0]])
    out = np.concatenate([src, dst_in[5:]])
    T.check_copy(src, dst_in, out, 40)
    out[7] = 1.0000000000000002                                                # one canary double overwritten
    with pytest.raises(AssertionError):
        T.check_copy(src, dst_in, out, 40)


def test_update_pass_references_against_python_loops():
    rng = np.random.default_rng(6)
    n = 9
    X, S, Cv = (rng.standard_normal(n + 2) for _ in range(3))
    x1, x2, s1, s2 = 0.7, 1 / 0.3, 1.9, 1 / 1.1
    Xo, So, Co = T.update_svec_ref(X, S, Cv, n, False, x1, x2, s1, s2)
    for i in range(n):
        assert Xo[i] == (float(X[i]) * x1) * x2 and So[i] == (float(S[i]) * s1) * s2 and Co[i] == 0.0
    assert np.array_equal(Xo[n:], X[n:]) and np.array_equal(So[n:], S[n:]) and np.array_equal(Co[n:], Cv[n:])
    Xz, Sz, Cz = T.update_svec_ref(-np.abs(X), S, None, n, True, x1, x2, s1, s2)
    assert Cz is None and Xz[:n].tobytes() == bytes(8 * n) and Sz[:n].tobytes() == bytes(8 * n)      # +0, not -0
    T.check_with_canary(Xo, Xo.copy(), n, "X")
    for at, v in ((3, np.nextafter(Xo[3], np.inf)), (n, 0.0), (n + 1, np.nextafter(Xo[n + 1], 0))):      # an element one ulp off; one canary double overwritten
        bad = Xo.copy()
        bad[at] = v
        with pytest.raises(AssertionError):
            T.check_with_canary(bad, Xo, n, "X")
    with pytest.raises(AssertionError):
        T.check_with_canary(-Xz, Xz, n, "X")                                   # -0 where +0 belongs
    m = 7
    b, y = rng.standard_normal(m + 2), rng.standard_normal(m + 2)
    na = 1 + rng.random(m)
    cs_old, ics_new = 3.3, 1 / 0.7
    bo, yo = T.update_cons_ref(b, y, na, m, 2, cs_old, ics_new)
    for i in range(m):
        assert bo[i] == 0.0 and yo[i] == ((float(y[i]) / float(na[i]) * cs_old) * float(na[i])) * ics_new
    assert np.array_equal(bo[m:], b[m:]) and np.array_equal(yo[m:], y[m:])
    bo, yo = T.update_cons_ref(None, y, None, m, 1, cs_old, ics_new)
    assert bo is None and not yo[:m].any() and np.array_equal(yo[m:], y[m:])
    bo, yo = T.update_cons_ref(b, y, None, m, 0, cs_old, ics_new)
    assert np.array_equal(yo, y) and not bo[:m].any()
    assert T.update_cons_ref(None, None, None, m, 0, cs_old, ics_new) == (None, None)
    v = rng.standard_normal(6)
    assert np.array_equal(T.scale_ref(v, 4, 0.3), np.array([float(a) * 0.3 for a in v[:4]] + list(v[4:])))
    dst = np.arange(10) + 0.5
    idx, val = np.array([7, 0, 3], np.int32), np.array([1.1, -2.2, 3.3])
    out = T.scatter_scaled_ref(dst, idx, val, 0.3)
    for i in range(10):
        assert out[i] == (float(val[list(idx).index(i)]) * 0.3 if i in idx else dst[i])


def test_hooks_refuse_malformed_input_before_anything_is_launched():
    """every refusal below is decided on the host, ahead of the first allocation: it needs no device"""
    import ctypes as C

    import cuadmm_amd
    lib = cuadmm_amd.load()
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    INVALID = -1                                              # CUADMM_ERR_INVALID (include/cuadmm_amd.h)
    rp, ci, av, y, Cv, X, idx = tiny_problem()
    L = rp.size - 1
    Rd1, Xb = np.zeros(L), np.zeros(L)

    def aty(idx, rp=rp, ci=ci):
        return lib.cuadmm_op_aty_xb_idx(L, y.size, P(rp), P(ci), P(av), P(y), P(Cv), P(X), 1.0, idx.size, P(idx), P(Rd1), P(Xb))
    for bad in (np.array([0, L], np.int32), np.array([-1], np.int32), np.array([3, 4, 3], np.int32)):
        assert aty(bad) == INVALID
    bad_ci = ci.copy()
    bad_ci[-1] = y.size
    assert aty(idx, ci=bad_ci) == INVALID
    bad_rp = rp.copy()
    bad_rp[4] = bad_rp[3] - 1
    assert aty(idx, rp=bad_rp) == INVALID

    S, sums, part, nparts = np.zeros(L), np.zeros(2), np.zeros(2 * 4), C.c_int(0)
    fused = np.zeros(6)

    def post(mode, idx, nfused):
        return lib.cuadmm_op_post_rest(mode, L, idx.size, P(idx), nfused, P(fused), P(X), P(X), P(Cv), P(Rd1), P(S), 1.0, 1.0, 0, P(sums), P(part), C.byref(nparts))
    none = np.zeros(0, np.int32)
    assert post(2, idx, 3) == INVALID and post(-1, idx, 3) == INVALID
    assert post(0, none, 0) == INVALID                        # nothing to do at all
    assert post(0, np.array([L], np.int32), 3) == INVALID and post(0, np.array([1, 1], np.int32), 3) == INVALID and post(0, idx, -1) == INVALID

    p = np.zeros(12)
    out = np.zeros(4 * 64 + 4)
    assert lib.cuadmm_op_reduce_quads(P(p), -1, P(p), 1, 2, 1, P(out), P(sums)) == INVALID
    assert lib.cuadmm_op_reduce_quads(P(p), 1, P(p), 1, -1, 1, P(out), P(sums)) == INVALID
    for n, stride, iters in ((3, 5, 1), (3, 4, 1), (3, 7, 1), (3, 6, 0), (3, 6, 65), (-1, 6, 1)):      # stride even and >= 2 n; iters in [1, 64]
        assert lib.cuadmm_op_reduce_quads_batch(P(p), P(p), n, stride, iters, P(out)) == INVALID

    rows, cl, bo, changed = np.arange(16, dtype=np.int32), np.zeros(32), np.zeros(16), C.c_int64(0)
    for nk, r in (([0, 1], rows), ([9, 1], rows), ([2, 8], np.where(rows == 15, 20, rows)), ([2, 1], np.where(rows == 1, -1, rows))):
        nk, r = np.array(nk, np.int32), np.ascontiguousarray(r, np.int32)
        assert lib.cuadmm_op_closed_rows(2, P(nk), P(r), 20, P(np.zeros(20)), P(np.zeros(20)), P(np.zeros(20)), P(cl), P(bo), C.byref(changed)) == INVALID

    assert lib.cuadmm_op_copy(P(p), 0, P(out)) == INVALID
    nbytes = np.array([8, -4], np.int64)
    ptrs = (C.c_void_p * 2)(p.ctypes.data, p.ctypes.data)
    assert lib.cuadmm_op_copy_multi(2, P(nbytes), ptrs, ptrs) == INVALID
    assert lib.cuadmm_op_copy_multi(0, P(nbytes), ptrs, ptrs) == INVALID and lib.cuadmm_op_copy_multi(7, P(nbytes), ptrs, ptrs) == INVALID
    assert lib.cuadmm_op_scale(P(p), 0, 2.0) == INVALID
    assert lib.cuadmm_op_update_svec(0, P(p), P(p), None, 0, 1.0, 1.0, 1.0, 1.0) == INVALID
    assert lib.cuadmm_op_update_cons(4, P(p), P(p), P(p), 3, 1.0, 1.0) == INVALID
    assert lib.cuadmm_op_update_cons(4, P(p), None, P(p), 1, 1.0, 1.0) == INVALID          # y is written: it has to be there
    assert lib.cuadmm_op_update_cons(4, P(p), P(p), None, 2, 1.0, 1.0) == INVALID
    val = np.zeros(3)
    for bad in (np.array([0, 12, 1], np.int32), np.array([0, -1, 1], np.int32), np.array([5, 2, 5], np.int32)):
        assert lib.cuadmm_op_scatter_scaled(12, P(p), 3, P(bad), P(val), 2.0) == INVALID
    assert b"bad arguments" in lib.cuadmm_last_error()
