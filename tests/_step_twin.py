"""numpy twin of the kernels behind the test hooks cuadmm_op_aty_xb_idx, _post_rest, _reduce_quads, _reduce_quads_batch, _closed_rows,
_copy, _copy_multi, _scale, _update_svec, _update_cons and _scatter_scaled (csrc/vec_kernels.hip; include/cuadmm_amd.h), with the
checkers tests/test_gpu_step_kernels.py runs on what the device returns.  tests/test_step_twin_host.py checks the twin itself and that
every checker refuses a corrupted result.

References are np.longdouble; the bounds are the derived ones of tests/test_gpu_iter_kernels.py, asserted per element:
  sparse dot product of n terms:  |got - ref| <= (n + 2) 2^-53 (sum |a_i x_i| + |c|)      (any summation order, with or without FMA)
  elementwise update:             2 - 4 ulp of the largest term, plus what the inputs' own bounds carry through
  sums over N terms:              (N + 2) 2^-53 sum |terms|, plus the terms' own bounds
  data movement, update passes:   the same BITS.  copy, copy_multi, gather_out, patch_b move bytes; scale, scatter_scaled, update_svec
                                  and update_cons hold only multiplications and one IEEE division -- (x x1) x2 and
                                  ((y / na cs_old) na) ics_new -- which nothing can contract to an FMA, so float64 numpy applying the
                                  same operations in the same order is the exact reference.
Sums of integer-valued doubles below 2^53 are exact in every association: their reference is Python's int.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
F64 = lambda a: np.asarray(a, dtype=np.float64)
QUAD_SEG = 16384                      # kQuadSeg: pairs per segment of reduce_quads
REC_FILL = 0xA5                       # every byte of a closed-block record the hook does not set
REC_FILL_DOUBLE = np.frombuffer(bytes([REC_FILL] * 8), np.float64)[0]


def post_grid(n):
    """workgroups of the list kernels' sums: one per 1 024 rows, at least 1, at most 2 048 (post_grid, csrc/vec_kernels.hip)"""
    return int(min(2048, max(1, (n + 1023) // 1024)))


def quad_segments(n1, n2):
    return max(1, (max(n1, n2) + QUAD_SEG - 1) // QUAD_SEG)


def same_bits(got, want, what):
    """raises unless the two arrays hold the same bytes; NaNs compare by their bits"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s against %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.nonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))[0]
    assert bad.size == 0, "%s: %d bytes differ, the first in element %d" % (what, bad.size, bad[0] // got.dtype.itemsize)


def within(got, ref, tol, what):
    """raises unless |got - ref| <= tol in every element (a NaN fails)"""
    err = np.abs(F64(np.asarray(got).astype(LD) - ref))
    bad = np.nonzero(~(err <= tol))[0]
    assert bad.size == 0, "%s: elements %s, errors %s, bounds %s" % (what, bad[:8], err[bad[:8]], np.asarray(tol)[bad[:8]])


def unlisted(n, idx):
    keep = np.ones(n, bool)
    keep[idx] = False
    return keep


def row_sums(rp, vals):
    """per-row sums of `vals` (any dtype) over a CSR row pointer; empty rows give 0"""
    out = np.zeros(rp.size - 1, vals.dtype)
    ne = rp[1:] > rp[:-1]
    if vals.size:
        out[ne] = np.add.reduceat(vals, rp[:-1][ne].astype(np.int64))
    return out


# ------------------------------------------------------------------------------------------------------------ aty_xb_idx
def aty_xb_ref(rp, ci, av, y, Cv, X, sig):
    """every row: Rd1 = At y - C and Xb = X + sig Rd1 in longdouble, each with its float64 bound"""
    n = (rp[1:] - rp[:-1]).astype(np.float64)
    prod = av.astype(LD) * y[ci].astype(LD)
    r = row_sums(rp, prod) - Cv.astype(LD)
    tol_r = (n + 2) * U * (F64(row_sums(rp, np.abs(prod))) + np.abs(Cv))
    xb = X.astype(LD) + LD(sig) * r
    tol_xb = abs(sig) * tol_r + 4 * U * np.maximum(np.abs(X), np.abs(sig * F64(r)))
    return r, tol_r, xb, tol_xb


def check_aty_xb_idx(rp, ci, av, y, Cv, X, sig, idx, Rd1_in, Xb_in, Rd1, Xb):
    L = rp.size - 1
    r, tol_r, xb, tol_xb = aty_xb_ref(rp, ci, av, y, Cv, X, sig)
    within(Rd1[idx], r[idx], tol_r[idx], "Rd1 on the listed rows")
    within(Xb[idx], xb[idx], tol_xb[idx], "Xb on the listed rows")
    empty = idx[rp[idx + 1] == rp[idx]]
    same_bits(Rd1[empty], 0.0 - Cv[empty], "Rd1 on listed empty rows (0 - C is exact)")
    rest = unlisted(L, idx)
    same_bits(Rd1[rest], Rd1_in[rest], "Rd1 outside the list")
    same_bits(Xb[rest], Xb_in[rest], "Xb outside the list")


# ------------------------------------------------------------------------------------------------------------- post_rest
def post_rest_ref(idx, Xp, Rd1, Cv, X0, inv_sig, tau_sig):
    """the listed rows in list order: S and the new X in longdouble with their bounds, and the two sums' terms with theirs"""
    xp, r1, c, x0 = Xp[idx], Rd1[idx], Cv[idx], X0[idx]
    s = LD(inv_sig) * (xp.astype(LD) - x0.astype(LD)) - r1.astype(LD)
    tol_s = 4 * U * np.maximum(np.abs(inv_sig * (xp - x0)), np.abs(r1)) + abs(inv_sig) * 2 * U * np.maximum(np.abs(xp), np.abs(x0))
    rd = r1.astype(LD) + s
    tol_rd = tol_s + 4 * U * np.maximum(np.abs(r1), np.abs(F64(s)))
    xn = x0.astype(LD) + LD(tau_sig) * rd
    tol_x = abs(tau_sig) * tol_rd + 4 * U * np.maximum(np.abs(x0), np.abs(tau_sig * F64(rd)))
    rdf = np.abs(F64(rd))
    cx = c.astype(LD) * xn
    return {"s": s, "tol_s": tol_s, "xn": xn, "tol_x": tol_x,
            "rd2": rd * rd, "tol_rd2": 2 * rdf * tol_rd + tol_rd * tol_rd + 2 * U * rdf * rdf,
            "cx": cx, "tol_cx": np.abs(c) * tol_x + 2 * U * np.abs(F64(cx))}


def sum_bound(n_terms, abs_sum, carried):
    return (n_terms + 2) * U * abs_sum + carried


def check_pair_sums(got2, ref, fused_pairs, what):
    """got2 against sum of the fused pairs (exact inputs) + sum of the listed rows' terms"""
    fp = fused_pairs.astype(LD).reshape(-1, 2)
    N = fp.shape[0] + ref["rd2"].size
    for k, (t, tt) in enumerate((("rd2", "tol_rd2"), ("cx", "tol_cx"))):
        want = np.sum(fp[:, k]) + np.sum(ref[t])
        tol = sum_bound(N, float(np.sum(np.abs(fp[:, k])) + np.sum(np.abs(ref[t]))), float(np.sum(ref[tt])))
        err = abs(float(LD(got2[k]) - want))
        assert err <= tol, "%s[%d]: %r against %r, error %g, bound %g" % (what, k, got2[k], float(want), err, tol)


def check_post_rest(mode, idx, fused_pairs, Xp, Rd1, Cv, X0, S0, inv_sig, tau_sig, use_quads, sums_in, X, S, sums, partials, nparts):
    L, nfused, grid = X0.size, fused_pairs.size // 2, (post_grid(idx.size) if idx.size else 0)
    ref = post_rest_ref(idx, Xp, Rd1, Cv, X0, inv_sig, tau_sig)
    rest = unlisted(L, idx)
    assert partials.size == 2 * (nfused + grid)
    assert nparts == (nfused + grid if use_quads else -1), "nparts_out %d" % nparts
    within(S[idx], ref["s"], ref["tol_s"], "S on the listed rows")
    same_bits(S[rest], S0[rest], "S outside the list")
    same_bits(partials[:2 * nfused], fused_pairs, "the fused blocks' pairs")
    if mode == 1:
        same_bits(X, X0, "X (mode 1 writes none)")
        same_bits(sums, sums_in, "sums2 (mode 1 writes none)")
        same_bits(partials[2 * nfused:], np.full(2 * grid, np.nan), "the partial pairs (mode 1 writes none)")
        return
    within(X[idx], ref["xn"], ref["tol_x"], "X on the listed rows")
    same_bits(X[rest], X0[rest], "X outside the list")
    host = partials.astype(LD).reshape(-1, 2).sum(axis=0)
    check_pair_sums(host, ref, fused_pairs, "the partial pairs summed on the host")
    if use_quads:
        same_bits(sums, sums_in, "sums2 (the caller reduces)")
    else:
        check_pair_sums(sums, ref, fused_pairs, "sums2")


# ---------------------------------------------------------------------------------------------------------- reduce_quads
def quads_exact(p1, p2):
    """[sum p2.x, sum p2.y, sum p1.x, sum p1.y] of integer-valued pairs, with Python ints"""
    out = []
    for p in (p2, p1):
        q = p.reshape(-1, 2)
        assert np.all(q == np.rint(q))
        out += [sum(int(v) for v in q[:, 0]), sum(int(v) for v in q[:, 1])]
    assert all(abs(v) < 2 ** 53 for v in out)
    return out


def check_quads_exact(p1, p2, out4, sums2=None):
    want = np.array([float(v) for v in quads_exact(p1, p2)])
    same_bits(out4 + 0.0, want + 0.0, "out4 = [sum p2.x, sum p2.y, sum p1.x, sum p1.y] (integers: exact)")      # + 0.0: one zero
    if sums2 is not None:
        same_bits(sums2, out4[2:4], "sums2 = out4[2:4]")


def check_quads_bound(p1, p2, out4, sums2=None):
    for k, q in enumerate((p2.reshape(-1, 2)[:, 0], p2.reshape(-1, 2)[:, 1], p1.reshape(-1, 2)[:, 0], p1.reshape(-1, 2)[:, 1])):
        want = np.sum(q.astype(LD))
        tol = sum_bound(q.size, float(np.sum(np.abs(q.astype(LD)))), 0.0)
        err = abs(float(LD(out4[k]) - want))
        assert err <= tol, "out4[%d]: %r against %r, error %g, bound %g" % (k, out4[k], float(want), err, tol)
    if sums2 is not None:
        same_bits(sums2, out4[2:4], "sums2 = out4[2:4]")


def check_quads_batch(out4, canary, singles):
    """out4: 4 iters + 4 doubles; singles[k]: the four scalars of iteration k from a launch of its own"""
    iters = len(singles)
    assert out4.size == 4 * iters + 4
    for k in range(iters):
        same_bits(out4[4 * k:4 * k + 4], singles[k], "iteration %d against a launch of its own" % k)
    same_bits(out4[4 * iters:], canary, "the canary behind out4")


# ----------------------------------------------------------------------------------------------------------- closed_rows
def closed_rows_ref(nk, rows, ax, as_, b, cl_in):
    """cl_out (16 per slot: A X of the slot's rows, then A (S - C)) and rec.b[0, 8) per slot; what no row fills keeps its bits"""
    nslots = nk.size
    cl = cl_in.copy().reshape(nslots, 16)
    bo = np.full((nslots, 8), REC_FILL_DOUBLE)
    r = rows.reshape(nslots, 8)
    for k in range(8):
        on = nk > k
        cl[on, k] = ax[r[on, k]]
        cl[on, 8 + k] = as_[r[on, k]]
        bo[on, k] = b[r[on, k]]
    return cl.reshape(-1), bo.reshape(-1)


def check_closed_rows(nk, rows, ax, as_, b, cl_in, cl_out, b_out, changed):
    cl, bo = closed_rows_ref(nk, rows, ax, as_, b, cl_in)
    same_bits(cl_out, cl, "cl_out")
    same_bits(b_out, bo, "rec.b")
    assert changed == 0, "%d record bytes outside b[0, nk) changed" % changed


# ------------------------------------------------------------------------------------------- copies and the update passes
def check_copy(src, dst_in, dst_out, nbytes, what="copy"):
    """the first nbytes bytes of dst_out are src's, every byte behind them (the canary) is dst_in's"""
    s, i, o = (np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in (src, dst_in, dst_out))
    assert i.size == o.size and o.size > nbytes and s.size >= nbytes
    same_bits(o[:nbytes], s[:nbytes], "%s: the data" % what)
    same_bits(o[nbytes:], i[nbytes:], "%s: the canary" % what)


def check_with_canary(got, want, n, what):
    """got, want: n elements followed by the canary, which `want` holds as it was uploaded"""
    same_bits(got[:n], want[:n], what)
    same_bits(got[n:], want[n:], "%s: the canary" % what)


def scale_ref(v, n, s):
    out = v.copy()
    out[:n] = v[:n] * s
    return out


def update_svec_ref(X, S, Cv, n, zero, x1, x2, s1, s2):
    """X <- (X x1) x2, S <- (S s1) s2 (zero: both <- +0), C <- +0 where given, on the first n elements"""
    Xo, So, Co = X.copy(), S.copy(), None if Cv is None else Cv.copy()
    Xo[:n] = 0.0 if zero else (X[:n] * x1) * x2
    So[:n] = 0.0 if zero else (S[:n] * s1) * s2
    if Co is not None:
        Co[:n] = 0.0
    return Xo, So, Co


def update_cons_ref(b, y, normA, m, ymode, cs_old, ics_new):
    """b <- +0 where given; y by ymode: 0 left, 1 <- +0, 2 <- ((y / normA cs_old) normA) ics_new"""
    bo, yo = None if b is None else b.copy(), None if y is None else y.copy()
    if bo is not None:
        bo[:m] = 0.0
    if ymode == 1:
        yo[:m] = 0.0
    elif ymode == 2:
        yo[:m] = ((y[:m] / normA[:m] * cs_old) * normA[:m]) * ics_new
    return bo, yo


def scatter_scaled_ref(dst, idx, val, s):
    out = dst.copy()
    out[idx] = val * s
    return out
