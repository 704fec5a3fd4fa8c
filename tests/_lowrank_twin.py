"""numpy twin of the per-block pivoted Cholesky (cuadmm_lowrank, cuadmm_op_block_lowrank: DESIGN.md, "Low-rank factors";
csrc/lowrank.hip), the four statements its results are held to, and the test matrices.

The twin runs the same algorithm with the same tie rule (the smallest index of the largest residual diagonal entry); it sums the products
of a column in numpy's order and updates d without an fma, so device and twin are not compared digit for digit: both are held to the
statements, which hold for any order of summation.

check_properties asserts, with E = M - L L' (formed in np.longdouble, so that the reference adds nothing), r the reported rank,
u = 2^-53 and b_i = (2 (r + 2) u + conv) (|m_ii| + sum_j L_ij^2) the residual-diagonal bound of row i:
  structure   the pivots are distinct rows, -1 beyond r; L[piv[j], j] > 0; L[piv[i], j] == 0.0 for i < j; columns >= r are zero
  residual    the kernel returns the computed d only through its sums, so the statement |E_ii - d_i| <= b_i is held in the forms that
  diagonal    can be read off them: |E_pp| <= b_p on pivot rows (d_p = 0); | sum |E_ii| - resid | <= sum b_i + n u resid over the rows
              not chosen (a sum of n terms of one sign carries at most n u relative, in any order); | min(0, min_i E_ii) - dneg | <=
              max b_i; flag 0: every remaining E_ii <= thr + b_i; flag 1: some remaining E_ii > thr - b_i, and r = min(n, rmax)
  PSD input   ||M - L L'||_F <= resid + 4 (n + 2) u tr M
  rank        flag 0 and r < n: lambda_{r+1}(M) <= n (thr + max b_i) + n u ||M||_F, the last term LAPACK's backward error of the
              reference eigenvalues; the callers add rank == r0 on the lowrank_* families
conv: a further relative error of m_ii, the L_ij^2, thr and the sums, for results the engine converted to the caller's units (0 for the
bare kernel).
"""
import numpy as np

from tests._infeas_twin import svec

INV_SQRT2 = 0.7071067811865476          # kLrInvSqrt2 (csrc/lowrank.hip)
U = 2.0 ** -53
RANGE_LO, RANGE_HI = 2.0 ** -500, 2.0 ** 500
COMPLETE, CAPPED, FREE, NOT_FACTORED = 0, 1, 2, 3
LD = np.longdouble
TOL = 1e-8                              # of every case below


def pack(M):
    """svec of M: row by row of the lower triangle, off-diagonal entries times sqrt(2)"""
    return svec(M)


def unpack(v, n):
    """the dense block as the kernel forms it: off-diagonal entries times one rounded constant"""
    ii, jj = np.tril_indices(n)
    w = np.where(ii == jj, v, v * INV_SQRT2)
    M = np.zeros((n, n))
    M[ii, jj] = w
    M[jj, ii] = w
    return M


def twin(M, tol, rmax):
    """(rank, resid, dneg, trace, flag, L (n, rc), piv (rc)) of one PSD block"""
    n = M.shape[0]
    rc = min(n, rmax)
    L, piv = np.zeros((n, rc)), np.full(rc, -1, np.int64)
    d = np.diag(M).copy()
    t = float(d.sum())
    with np.errstate(invalid="ignore"):
        amax = float(np.abs(M).max())
    if not (amax <= RANGE_HI and (amax >= RANGE_LO or amax == 0.0)):
        return 0, float("nan"), 0.0, t, NOT_FACTORED, L, piv
    thr = tol * max(float(d.max()), 0.0)
    alive = np.ones(n, bool)
    r, flag = 0, COMPLETE
    while True:
        cand = np.where(alive, d, -np.inf)
        p = int(np.argmax(cand))                    # the first index of the maximum
        dp = cand[p]
        if not dp > thr:
            break
        if r == rc:
            flag = CAPPED
            break
        s = np.sqrt(dp)
        col = (M[:, p] - L[:, :r] @ L[p, :r]) / s
        col[~alive] = 0.0
        col[p] = s
        L[:, r], piv[r] = col, p
        alive[p] = False
        d[alive] -= col[alive] ** 2
        r += 1
    rest = d[alive]
    return r, float(np.abs(rest).sum()), float(min(0.0, rest.min())) if rest.size else 0.0, t, flag, L, piv


def check_properties(M, tol, rmax, rank, resid, dneg, flag, L, piv, psd=True, conv=0.0, what=""):
    """asserts the four statements of the module docstring for one factored block; L: (n, min(n, rmax)), piv: min(n, rmax) ints"""
    n = M.shape[0]
    rc = min(n, rmax)
    r = int(rank)
    assert flag in (COMPLETE, CAPPED) and 0 <= r <= rc and L.shape == (n, rc) and len(piv) == rc, (what, flag, r, L.shape)
    p = np.asarray(piv[:r], np.int64)
    # ---- structure
    assert np.all(np.asarray(piv[r:]) == -1) and np.all((p >= 0) & (p < n)) and len(set(p.tolist())) == r, (what, "pivots", piv)
    assert np.all(L[:, r:] == 0.0), (what, "columns beyond the rank")
    for j in range(r):
        assert L[p[j], j] > 0 and np.all(L[p[:j], j] == 0.0), (what, "structure of column", j)
    # ---- residual diagonal
    Ll = L[:, :r].astype(LD)
    dM = np.diag(M)
    sq = np.sum(Ll * Ll, axis=1)
    Eii = (dM.astype(LD) - sq).astype(np.float64)
    b = (2 * (r + 2) * U + conv) * (np.abs(dM) + sq.astype(np.float64))
    rest = np.ones(n, bool)
    rest[p] = False
    assert np.all(np.abs(Eii[p]) <= b[p]), (what, "pivot rows", np.max(np.abs(Eii[p]) - b[p]))
    thr = tol * max(float(dM.max()), 0.0)
    slack = float(b[rest].sum()) + n * U * abs(resid) + conv * abs(resid)
    assert abs(float(np.abs(Eii[rest]).sum()) - resid) <= slack, (what, "resid", resid, float(np.abs(Eii[rest]).sum()), slack)
    bmax = float(b[rest].max()) if rest.any() else 0.0
    emin = min(0.0, float(Eii[rest].min())) if rest.any() else 0.0
    assert dneg <= 0.0 and abs(emin - dneg) <= bmax + conv * abs(dneg), (what, "dneg", dneg, emin, bmax)
    if flag == COMPLETE:
        assert np.all(Eii[rest] <= thr * (1 + conv) + b[rest]), (what, "flag 0", float(np.max(Eii[rest] - thr - b[rest])))
    else:
        assert r == rc and np.any(Eii[rest] > thr * (1 - conv) - b[rest]), (what, "flag 1")
    if not psd:
        return
    # ---- PSD input
    Ml = M.astype(LD)
    err = float(np.sqrt(np.sum((Ml - Ll @ Ll.T) ** 2)))
    t = float(dM.sum())
    assert err <= resid + 4 * (n + 2) * U * t * (1 + conv), (what, "PSD input", err, resid, 4 * (n + 2) * U * t)
    # ---- rank
    if flag == COMPLETE and r < n:
        lam = np.linalg.eigvalsh(M)[::-1]
        assert lam[r] <= n * (thr + bmax) + n * U * float(np.linalg.norm(M)), (what, "rank", r, lam[r], thr)


# ---- the test matrices ----------------------------------------------------------------------------------------------------
def _low_rank(n, r0, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((n, r0)))
    lam = np.geomspace(1.0, 1e-3, r0) if r0 > 1 else np.ones(1)
    M = (Q * lam) @ Q.T
    return unpack(svec((M + M.T) / 2), n)


# size -> (rmax, the families run at it; None: all).  One wavefront up to 32, a workgroup of 256 beyond (first and second pass of its strided
# loops); 300: the cap below the rank (flag 1 on full, flag 0 on lowrank_5); 1100: beyond what cuadmm_lambda_min refines.
SIZES = {1: (1, None), 2: (2, None), 3: (3, None), 31: (31, None), 32: (32, None), 33: (33, None), 64: (64, None), 65: (65, None), 130: (130, None),
         300: (8, ("full", "lowrank_5")), 1100: (4, ("lowrank_2",))}
LAUNCHES = {"wavefront": [1, 2, 3, 31, 32], "workgroup": [33, 64, 65, 130], "capped": [300], "large": [1100]}      # one op call each
_cases = {}


def cases(n):
    """[dict(n, family, M as the kernel will unpack it, vec its svec, r0 or None, psd)] of one size, built once and left alone"""
    if n in _cases:
        return _cases[n]
    rng = np.random.default_rng(1000 + n)
    out = []
    only = SIZES[n][1]

    def add(family, M, r0=None, psd=True):
        if only is None or family in only:
            out.append(dict(n=n, family=family, M=M, vec=pack(M), r0=r0, psd=psd))

    base2 = None
    for r0 in (1, 2, 5):
        if r0 <= n:
            M = _low_rank(n, r0, rng)
            add("lowrank_%d" % r0, M, r0)
            if r0 == 2:
                base2 = M
    if only is None or "full" in only:
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        F = (Q * (1.0 + rng.random(n))) @ Q.T
        add("full", unpack(svec((F + F.T) / 2), n), n)
    add("identity", np.eye(n), n)
    add("zero", np.zeros((n, n)), 0)
    I = _low_rank(n, min(n, 2), rng)
    I[n // 2, n // 2] = -0.25
    add("indef", I, None, psd=False)
    N = np.eye(n)
    N[n - 1, 0] = N[0, n - 1] = np.nan
    add("nan", N, None, psd=False)
    if base2 is not None:
        add("scaled_down", base2 * 2.0 ** -400, 2)
        add("scaled_up", base2 * 2.0 ** 400, 2)
    _cases[n] = out
    return out


def split(blk, rmax, per_block, L, piv):
    """per block (rank, resid, dneg, trace, flag, L_k (n_k, rc_k), piv_k) from the arrays of cuadmm_lowrank / cuadmm_op_block_lowrank"""
    pb = np.asarray(per_block).reshape(-1, 6)
    out = []
    for k, n in enumerate(blk):
        n = int(n)
        rc = min(n, rmax) if n > 0 else 0
        o = int(pb[k, 5])
        Lk = L[o:o + max(n, 0) * rc].reshape(rc, max(n, 0)).T
        out.append((int(pb[k, 0]), float(pb[k, 1]), float(pb[k, 2]), float(pb[k, 3]), int(pb[k, 4]), Lk, piv[o:o + rc]))
    return out


def lowrank_size(blk, rmax):
    return int(sum(int(n) * min(int(n), rmax) for n in blk if n > 0))
