"""Op-level tests of the kernels of csrc/vec_kernels.hip that only whole solves reached: the fused step's list kernels (aty_xb_idx,
post_idx), the quad sums (reduce_quads, its batch form), the closed blocks' row copies, the copies behind checkpoint and rollback,
and the update passes of cuadmm_update_bC -- through the test hooks cuadmm_op_aty_xb_idx, _post_rest, _reduce_quads,
_reduce_quads_batch, _closed_rows, _copy, _copy_multi, _scale, _update_svec, _update_cons and _scatter_scaled.

References and bounds: tests/_step_twin.py (np.longdouble with the derived bounds of tests/test_gpu_iter_kernels.py; Python ints for
sums of integers; the sibling hook for "the same bits as one launch per iteration"; float64 in the same order for the passes that only
multiply and divide).  Every size is the smallest that reaches the edge its case is named for.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd._lib import check
from tests import _step_twin as T

pytestmark = pytest.mark.gpu

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
ERR_INVALID = -1                                          # CUADMM_ERR_INVALID (include/cuadmm_amd.h)
NAN4 = np.full(4, np.nan)


def distinct(n, sign=1.0):
    """finite, pairwise different fill values: a partial or misplaced write shows"""
    return sign * (np.arange(n, dtype=np.float64) + 0.25)


# ------------------------------------------------------------------------------------------------------------ aty_xb_idx
LIST_PASS = 4096 * 256                                    # rows one pass of the list kernel's capped grid covers


@functools.lru_cache(maxsize=None)
def aty_problem(L):
    rng = np.random.default_rng(L)
    lengths = rng.integers(0, 4, L)
    lengths[[0, L // 2, L - 1]] = 40
    lengths[[1, L - 2]] = 0
    rp = np.zeros(L + 1, np.int32)
    rp[1:] = np.cumsum(lengths)
    m = 500
    ci = rng.integers(0, m, rp[-1]).astype(np.int32)
    out = (rp, ci, rng.standard_normal(rp[-1]), rng.standard_normal(m), rng.standard_normal(L), rng.standard_normal(L))
    for a in out:
        a.setflags(write=False)
    return out


def row_list(L, nidx, permuted, seed):
    rng = np.random.default_rng(seed)
    idx = rng.choice(L, nidx, replace=False)
    if nidx >= 5:                                          # the rows of 40 and the empty ones are on the list
        idx = np.concatenate([[0, 1, L // 2, L - 2, L - 1], np.setdiff1d(idx, [0, 1, L // 2, L - 2, L - 1])[:nidx - 5]])
    idx = np.sort(idx)
    return (rng.permutation(idx) if permuted else idx).astype(np.int32)


def run_aty_xb_idx(L, nidx, permuted):
    rp, ci, av, y, Cv, X = aty_problem(L)
    idx = row_list(L, nidx, permuted, nidx)
    assert idx.size == nidx and np.unique(idx).size == nidx
    sig = 1.7
    Rd1_in, Xb_in = distinct(L), distinct(L, -1.0)
    Rd1, Xb = Rd1_in.copy(), Xb_in.copy()
    check(cuadmm_amd.load().cuadmm_op_aty_xb_idx(L, y.size, P(rp), P(ci), P(av), P(y), P(Cv), P(X), sig, nidx, P(idx), P(Rd1), P(Xb)))
    T.check_aty_xb_idx(rp, ci, av, y, Cv, X, sig, idx, Rd1_in, Xb_in, Rd1, Xb)


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("nidx", [1, 255, 256, 257, 1025])
def test_aty_xb_idx_writes_the_listed_rows_and_no_other(nidx, permuted):
    run_aty_xb_idx(3000, nidx, permuted)


def test_aty_xb_idx_second_pass_of_the_capped_grid():
    run_aty_xb_idx(LIST_PASS + 1 + 1000, LIST_PASS + 1, True)


# ------------------------------------------------------------------------------------------------------------- post_rest
POST_BIG = 2048 * 1024 + 77                               # more rows than the 2 048 workgroups cover in one pass
FUSED3 = np.array([3.5, -1.25, 0.75, 2.0, 1e-3, -4.0])


@functools.lru_cache(maxsize=None)
def post_problem(L, nidx):
    rng = np.random.default_rng(L + nidx)
    out = tuple(rng.standard_normal(L) for _ in range(5)) + (rng.permutation(L)[:nidx].astype(np.int32),)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("use_quads", [0, 1])
@pytest.mark.parametrize("nidx,nfused", [(0, 3), (1, 0), (1, 3), (1025, 0), (1025, 3), (POST_BIG, 0), (POST_BIG, 3)])
@pytest.mark.parametrize("mode", [0, 1])
def test_post_rest_rows_sums_and_partial_pairs(mode, nidx, nfused, use_quads):
    L = 3000 if nidx < 3000 else nidx + 1000
    Xp, Rd1, Cv, X0, S0, idx = post_problem(L, nidx)
    fused = FUSED3[:2 * nfused].copy()
    inv_sig, tau_sig = 1 / 1.3, 1.618 * 1.3
    sums_in = np.frombuffer(np.array([0x7ff8000000c0ffee, 0x7ff8000000c0ffef], np.uint64).tobytes(), np.float64)
    X, S, sums = X0.copy(), S0.copy(), sums_in.copy()
    partials = np.zeros(2 * (nfused + (T.post_grid(nidx) if nidx else 0)))
    nparts = C.c_int(-2)
    check(cuadmm_amd.load().cuadmm_op_post_rest(mode, L, nidx, P(idx), nfused, P(fused), P(Xp), P(Rd1), P(Cv), P(X), P(S), inv_sig, tau_sig, use_quads,
                                                P(sums), P(partials), C.byref(nparts)))
    T.check_post_rest(mode, idx, fused, Xp, Rd1, Cv, X0, S0, inv_sig, tau_sig, use_quads, sums_in, X, S, sums, partials, nparts.value)


# ---------------------------------------------------------------------------------------------------------- reduce_quads
def reduce_quads_gpu(p1, p2, with_scratch=1, pad_pairs=2):
    out4, sums2 = np.zeros(4), np.zeros(2)
    rc = cuadmm_amd.load().cuadmm_op_reduce_quads(P(p1), p1.size // 2, P(p2), p2.size // 2, pad_pairs, with_scratch, P(out4), P(sums2))
    return rc, out4, sums2


def pairs(kind, n, rng):
    if kind == "int":
        return rng.integers(-2 ** 20, 2 ** 20 + 1, 2 * n).astype(np.float64)
    return rng.standard_normal(2 * n)


QUAD_SIZES = [(1, 1), (1023, 1000), (1024, 1024), (1025, 1), (2049, 2048), (16383, 16383), (16384, 16384), (16385, 16384), (16385, 16385),
              (18432, 16384), (32768, 32768), (32769, 20000), (100003, 100000)]


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("n1,n2", QUAD_SIZES)
def test_reduce_quads_segments_order_and_scratch(n1, n2, kind):
    rng = np.random.default_rng(n1 + 7 * n2)
    p1, p2 = pairs(kind, n1, rng), pairs(kind, n2, rng)
    rc, out4, sums2 = reduce_quads_gpu(p1, p2)
    check(rc)
    (T.check_quads_exact if kind == "int" else T.check_quads_bound)(p1, p2, out4, sums2)
    rc0, out4_0, sums2_0 = reduce_quads_gpu(p1, p2, with_scratch=0)
    if T.quad_segments(n1, n2) == 1:                       # one segment: the scratch is not looked at and may be missing
        check(rc0)
        T.same_bits(out4_0, out4, "out4 without scratch")
        T.same_bits(sums2_0, sums2, "sums2 without scratch")
    else:                                                  # refused before anything is launched
        assert rc0 == ERR_INVALID
        T.same_bits(out4_0, NAN4, "out4 after the refusal")
        T.same_bits(sums2_0, NAN4[:2], "sums2 after the refusal")
    # the two sides swapped: n1 and n2 on the other side of every guard
    rc, out4s, sums2s = reduce_quads_gpu(p2, p1)
    check(rc)
    T.same_bits(out4s, out4[[2, 3, 0, 1]], "out4 with p1 and p2 swapped")
    T.same_bits(sums2s, out4[0:2], "sums2 with p1 and p2 swapped")


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("n", [1, 1025, 16384, 16385, 32769])
def test_reduce_quads_batch_has_the_bits_of_one_launch_per_iteration(n, iters, kind):
    rng = np.random.default_rng(n + iters)
    stride = 2 * n + 2
    p1, p2 = (np.full((iters, stride), np.nan) for _ in range(2))
    for k in range(iters):
        p1[k, :2 * n], p2[k, :2 * n] = pairs(kind, n, rng), pairs(kind, n, rng)
    canary = np.array([1.5, -2.5, np.nan, 4.5])
    out4 = np.concatenate([np.full(4 * iters, np.nan), canary])
    check(cuadmm_amd.load().cuadmm_op_reduce_quads_batch(P(p1), P(p2), n, stride, iters, P(out4)))
    singles = []
    for k in range(iters):
        a, b = p1[k, :2 * n].copy(), p2[k, :2 * n].copy()
        rc, single, _ = reduce_quads_gpu(a, b)
        check(rc)
        singles.append(single)
        (T.check_quads_exact if kind == "int" else T.check_quads_bound)(a, b, out4[4 * k:4 * k + 4])
    T.check_quads_batch(out4, canary, singles)


# ----------------------------------------------------------------------------------------------------------- closed_rows
def run_closed_rows(nk, seed):
    rng = np.random.default_rng(seed)
    nslots, m = nk.size, 5000
    rows = np.stack([rng.choice(m, 8, replace=False) for _ in range(nslots)]).astype(np.int32).reshape(-1)
    for s in range(nslots):
        rows[8 * s + nk[s]:8 * s + 8] = -12345                # behind nk: never read
    ax, as_, b = (rng.standard_normal(m) for _ in range(3))
    cl_in = distinct(16 * nslots)
    cl_out, b_out, changed = cl_in.copy(), np.zeros(8 * nslots), C.c_int64(-1)
    check(cuadmm_amd.load().cuadmm_op_closed_rows(nslots, P(nk), P(rows), m, P(ax), P(as_), P(b), P(cl_out), P(b_out), C.byref(changed)))
    T.check_closed_rows(nk, np.where(rows < 0, 0, rows), ax, as_, b, cl_in, cl_out, b_out, changed.value)


@pytest.mark.parametrize("nslots", [1, 31, 32, 33, 1000])
def test_closed_rows_fill_nk_slots_and_leave_the_record_alone(nslots):
    if nslots < 8:
        for v in range(1, 9):                              # every nk, one record each
            run_closed_rows(np.full(nslots, v, np.int32), v)
        return
    rng = np.random.default_rng(nslots)
    nk = rng.permutation(np.arange(nslots) % 8 + 1).astype(np.int32)
    assert set(nk) == set(range(1, 9))
    run_closed_rows(nk, nslots)


# ---------------------------------------------------------------------------------------------------------------- copies
COPY_PASS = 2048 * 256                                    # double2 words one pass of copy_kernel's capped grid moves


@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 2 * COPY_PASS, 4 * COPY_PASS + 3])
def test_copy_odd_lengths_and_the_two_in_flight_loop(n):
    rng = np.random.default_rng(n)
    src = rng.standard_normal(n)
    dst_in = distinct(n + 4, -1.0)
    dst = dst_in.copy()
    check(cuadmm_amd.load().cuadmm_op_copy(P(src), n, P(dst)))
    T.check_copy(src, dst_in, dst, 8 * n)


def copy_multi_gpu(lens, seed=0):
    rng = np.random.default_rng(seed + sum(lens))
    count = len(lens)
    srcs = [rng.integers(1, 255, max(n, 1)).astype(np.uint8) for n in lens]
    dst_in = [np.concatenate([np.full(n, 0xEE, np.uint8), np.arange(32, dtype=np.uint8) + 0x40 + q]) for q, n in enumerate(lens)]
    dsts = [d.copy() for d in dst_in]
    nbytes = np.array(lens, np.int64)
    sp = (C.c_void_p * count)(*[s.ctypes.data for s in srcs])
    dp = (C.c_void_p * count)(*[d.ctypes.data for d in dsts])
    rc = cuadmm_amd.load().cuadmm_op_copy_multi(count, P(nbytes), sp, dp)
    return rc, srcs, dst_in, dsts


COPY_MULTI = {
    "one job, a 4-byte tail": [20],
    "an empty job before a 12-byte tail": [0, 4096 + 12],
    "nothing of 16 bytes: the launch still happens": [4, 8, 12],
    "a 4-byte job between empty ones": [0, 4, 0],
    "all but one empty": [0, 0, 16, 0],
    "2 m + 2 doubles for odd m, tails, an empty job": [8 * (2 * 1001 + 2), 12, 0, 4096 + 12, 8],
    "six jobs, the first longer than one pass": [COPY_PASS * 16 + 20, 0, 4, 20, 16, 4096 + 12],
    "nothing to do": [0, 0],
}


@pytest.mark.parametrize("name", list(COPY_MULTI))
def test_copy_multi_tails_empty_jobs_and_canaries(name):
    lens = COPY_MULTI[name]
    rc, srcs, dst_in, dsts = copy_multi_gpu(lens)
    check(rc)
    for q, n in enumerate(lens):
        T.check_copy(srcs[q], dst_in[q], dsts[q], n, "job %d of %s" % (q, lens))


def test_copy_multi_covers_every_job_count_and_refuses_a_ragged_length():
    assert sorted({len(v) for v in COPY_MULTI.values()}) == [1, 2, 3, 4, 5, 6]
    rc, _, dst_in, dsts = copy_multi_gpu([16, 6])
    assert rc == ERR_INVALID
    for a, b in zip(dst_in, dsts):
        T.same_bits(b, a, "a destination of the refused call")


@pytest.mark.parametrize("n", [1, 257, 300001])
def test_scale_is_the_float64_product(n):
    rng = np.random.default_rng(n)
    v_in = np.concatenate([rng.standard_normal(n), distinct(4)])
    v = v_in.copy()
    check(cuadmm_amd.load().cuadmm_op_scale(P(v), n, 0.3))
    T.check_with_canary(v, T.scale_ref(v_in, n, 0.3), n, "v s")


# ---------------------------------------------------------------------------------------------------------- update passes
# (x1, x2, s1, s2) as cuadmm_update_bC and cuadmm_update_A pass them: 1 or the old scale, then one over the new scale
SVEC_SCALARS = [(1.0, 1 / 3.7, 1.0, 1 / 0.013), (41.3, 1 / 3.7, 0.77, 1 / 0.013), (1.0, 1.0 / 3.0, 1.0, 1e-3)]


@pytest.mark.parametrize("n", [1, 2, 3, 1023, 1024, 1025, 4 * COPY_PASS + 5])
@pytest.mark.parametrize("zero", [0, 1])
@pytest.mark.parametrize("with_c", [0, 1])
def test_update_svec_bits_and_the_pad_behind(with_c, zero, n):
    rng = np.random.default_rng(n)
    X0, S0 = (np.concatenate([rng.standard_normal(n), distinct(2)]) for _ in range(2))
    C0 = np.concatenate([rng.standard_normal(n), distinct(2, -1.0)]) if with_c else None
    X0[0] = -abs(X0[0])                                    # zero: +0 in place of a negative value, too
    for x1, x2, s1, s2 in SVEC_SCALARS:
        X, S, Cv = X0.copy(), S0.copy(), None if C0 is None else C0.copy()
        check(cuadmm_amd.load().cuadmm_op_update_svec(n, P(X), P(S), P(Cv), zero, x1, x2, s1, s2))
        Xr, Sr, Cr = T.update_svec_ref(X0, S0, C0, n, bool(zero), x1, x2, s1, s2)
        T.check_with_canary(X, Xr, n, "X")
        T.check_with_canary(S, Sr, n, "S")
        if with_c:
            T.check_with_canary(Cv, Cr, n, "C")


@pytest.mark.parametrize("m", [1, 255, 256, 257, 100001])
@pytest.mark.parametrize("ymode", [0, 1, 2])
@pytest.mark.parametrize("with_b", [0, 1])
def test_update_cons_bits_and_the_pad_behind(with_b, ymode, m):
    lib = cuadmm_amd.load()
    rng = np.random.default_rng(m)
    y0 = np.concatenate([rng.standard_normal(m), distinct(2)])
    b0 = np.concatenate([rng.standard_normal(m), distinct(2, -1.0)]) if with_b else None
    normA = 1.0 + 3.0 * rng.random(m)
    cs_old, ics_new = 0.77, 1 / 0.013
    b, y = None if b0 is None else b0.copy(), y0.copy()
    check(lib.cuadmm_op_update_cons(m, P(b), P(y), P(normA), ymode, cs_old, ics_new))
    br, yr = T.update_cons_ref(b0, y0, normA, m, ymode, cs_old, ics_new)
    T.check_with_canary(y, yr, m, "y")
    if with_b:
        assert not b[:m].any()
        T.check_with_canary(b, br, m, "b")
    if ymode == 0:                                         # y and normA are not looked at: the engine passes neither
        b = None if b0 is None else b0.copy()
        check(lib.cuadmm_op_update_cons(m, P(b), None, None, 0, cs_old, ics_new))
        if with_b:
            T.check_with_canary(b, br, m, "b without y")


@pytest.mark.parametrize("n", [0, 1, 257, 5000])
def test_scatter_scaled_targets_and_no_other_slot(n):
    rng = np.random.default_rng(n)
    length = 5000
    dst_in = distinct(length)
    idx = rng.permutation(length)[:n].astype(np.int32)
    val = rng.standard_normal(n)
    dst = dst_in.copy()
    check(cuadmm_amd.load().cuadmm_op_scatter_scaled(length, P(dst), n, P(idx), P(val), 1 / 3.7))
    T.same_bits(dst, T.scatter_scaled_ref(dst_in, idx, val, 1 / 3.7), "dst")
    T.same_bits(dst[T.unlisted(length, idx)], dst_in[T.unlisted(length, idx)], "the slots no index names")
    T.same_bits(dst[idx], val * (1 / 3.7), "the targets")
