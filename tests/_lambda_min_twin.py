"""numpy twin of the certified lambda_min (cuadmm_lambda_min, cuadmm_op_block_lambda_min: DESIGN.md, "Certified lambda_min";
csrc/lambda_min.hip), the two properties its results are held to, and the test matrices.

The twin brackets -lambda_min(M) between nu_floor = (n + 2) 2^-52 ||M||_F and the Gershgorin value nu_max and bisects geometrically on
the shift mu, a trial being numpy.linalg.cholesky(M + mu I); the margin of a success is the library's cuadmm_lambda_min_margin.

Properties, with lam = eigvalsh(M).min() and e = n 2^-52 ||M||_F (LAPACK's backward error with p(n) = n; both are passed in, so that a
matrix whose lambda_min is known exactly is held to e = 0):
  validity    lo <= lam + e
  tightness   flag 0: lo >= rho_T x - m(n, t, |x|) with x = min(lam - e, -nu_floor), rho_T = (nu_max / nu_floor)^(2^-T);
              flag 1: lam >= -nu_floor - m(n, t, nu_floor) - e
Device and twin are not compared digit for digit: a trial whose shift lies within rounding of -lambda_min may go either way.
"""
import ctypes as C

import numpy as np

import cuadmm_amd
from tests._infeas_twin import svec

INV_SQRT2 = 0.7071067811865476          # kLmInvSqrt2 (csrc/lambda_min.hip)
EPS = 2.0 ** -52
N_LDS, N_MAX = 200, 1024                # kLmLds, kLmMax (csrc/lambda_min.h)
RANGE_LO, RANGE_HI = 2.0 ** -500, 2.0 ** 500
REFINED, AT_FLOOR, FREE, UNREFINED = 0, 1, 2, 3


def margin(n, t, mu):
    return float(cuadmm_amd.load().cuadmm_lambda_min_margin(int(n), C.c_double(t), C.c_double(mu)))


def unpack(v, n):
    """the dense block as the kernel forms it: off-diagonal entries times one rounded constant"""
    ii, jj = np.tril_indices(n)
    w = np.where(ii == jj, v, v * INV_SQRT2)
    M = np.zeros((n, n))
    M[ii, jj] = w
    M[jj, ii] = w
    return M


def bracket(M):
    """t, f, nu_floor, nu_max of the block"""
    n = M.shape[0]
    d = np.diag(M)
    A = np.abs(M)
    g = float(np.min(d - (A.sum(axis=1) - np.abs(d))))
    eps = (n + 2) * EPS
    return float(d.sum()), float(np.linalg.norm(M)), eps * float(np.linalg.norm(M)), max(0.0, -g) + eps * float(A.sum())


def _trial(M, mu):
    try:
        with np.errstate(all="ignore"):
            R = np.linalg.cholesky(M + mu * np.eye(M.shape[0]))
        return bool(np.all(np.isfinite(R)) and np.all(np.diag(R) > 0))
    except np.linalg.LinAlgError:
        return False


def twin(M, T):
    """(lo, hi, flag) of one PSD block"""
    n = M.shape[0]
    t, f, nu_floor, nu_max = bracket(M)
    amax = float(np.abs(M).max())
    if n > N_MAX or not (amax <= RANGE_HI and (amax >= RANGE_LO or amax == 0.0)):
        return -nu_max, float(np.diag(M).min()), UNREFINED
    if _trial(M, nu_floor):
        return max(-nu_floor - margin(n, t, nu_floor), -nu_max), float(np.diag(M).min()), AT_FLOOR
    a, c, won = nu_floor, nu_max, None
    for _ in range(T):
        if not c > a:
            break
        mu = np.sqrt(a) * np.sqrt(c)
        if not a < mu < c:
            break
        if _trial(M, mu):
            c = won = mu
        else:
            a = mu
    lo = -nu_max if won is None else max(-won - margin(n, t, won), -nu_max)
    return lo, -a, REFINED


def reference(M):
    """lam, e of the module docstring"""
    return float(np.linalg.eigvalsh(M).min()), M.shape[0] * EPS * float(np.linalg.norm(M))


def check_properties(M, T, lo, hi, flag, lam, e, what=""):
    """asserts validity and tightness of (lo, hi, flag) for the block M with reference lam, e"""
    n = M.shape[0]
    t, f, nu_floor, nu_max = bracket(M)
    assert np.isfinite(lo) and lo <= lam + e, (what, "validity", lo, lam, e)
    if flag == UNREFINED:
        return
    assert flag in (REFINED, AT_FLOOR), (what, flag)
    if flag == AT_FLOOR:
        assert lam >= -nu_floor - margin(n, t, nu_floor) - e, (what, "flag 1", lam, nu_floor)
        return
    rho = (nu_max / nu_floor) ** (2.0 ** -T) if nu_max > nu_floor > 0 else 1.0
    x = min(lam - e, -nu_floor)
    assert lo >= rho * x - margin(n, t, abs(x)), (what, "tightness", lo, rho, x, lam, e, nu_floor, nu_max)
    assert lo <= hi <= 0, (what, "hi", lo, hi)


# ---- the test matrices ----------------------------------------------------------------------------------------------------
FAMILIES = ("diagonal", "psd_half_rank", "indef_1e-3", "indef_1e-9", "neg_def", "zero", "tiny")
SIZE_CLASSES = {                        # one op call each: the kernel's launches by size (csrc/lambda_min.h)
    "wavefront": [1, 2, 3, 8, 9, 16, 17, 32],
    "lds64": [33, 64],
    "lds128": [65],
    "lds200": [N_LDS - 1, N_LDS],
    "global": [N_LDS + 1, 230],
}


def _with_spectrum(n, lam, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    M = (Q * lam) @ Q.T
    return (M + M.T) / 2


def make_matrix(n, family, rng):
    """(M as the kernel will unpack it, its svec, exactly known lambda_min or None)"""
    exact = None
    if family == "diagonal":
        d = rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3)
        M, exact = np.diag(d), float(d.min())
    elif family == "psd_half_rank":
        V = rng.standard_normal((n, n // 2))
        M = V @ V.T
    elif family.startswith("indef"):
        lam = 0.1 + rng.random(n)
        lam[0] = -float(family[6:])
        M = _with_spectrum(n, lam, rng)
    elif family == "neg_def":
        G = rng.standard_normal((n, n))
        M = -(G @ G.T / n + 0.1 * np.eye(n))
    elif family == "zero":
        M, exact = np.zeros((n, n)), 0.0
    else:
        G = rng.standard_normal((n, n))
        M = 1e-300 * (G + G.T)
    v = svec(M)
    return unpack(v, n), v, exact


_cases = {}


def cases(name):
    """[(n, family, M, svec, exact)] of a size class, built once"""
    if name not in _cases:
        rng = np.random.default_rng(sum(map(ord, name)))
        _cases[name] = [(n, fam) + make_matrix(n, fam, rng) for n in SIZE_CLASSES[name] for fam in FAMILIES]
    return _cases[name]
