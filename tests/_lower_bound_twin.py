"""numpy twin of the certified lower bound (cuadmm_lower_bound, option "gap_check": DESIGN.md, "Certified lower bound";
csrc/engine_reports.hip: lb_eval, lb_step) and problems with a known optimum.

The bound at any y, in the caller's units, with S^ = C - A'y:

    LB(y) = b'y - sum_k R_k nubar_k,   nubar_k = ||P+(-S^_k)||_F + PROJ_ERR sqrt(len_k) ||S^_k||_F   (PSD block)
                                       nubar_k = ||S^_k||_2                                            (unconstrained block)

Here P+ is numpy.linalg.eigvalsh per block and the two final sums run in np.longdouble.  The in-solve rule hooks
oracle.cuadmm_oracle.OracleSolver's ``stage_hook`` at the end of every iteration, as tests/_infeas_twin.py does.

Fixture with a known optimum (make_opt_fixture): per PSD block X* = Q1 D1 Q1' and S* = Q2 D2 Q2' on complementary eigenspaces of one
random orthogonal Q; unconstrained block: S* = 0, x* random; y* random, C = A'y* + S*, b = A X*.  Then <C, X*> = b'y* + <S*, X*> =
b'y*: X* and (y*, S*) are optimal and p* = b'y*.  R_k = 1.5 tr X*_k (1.5 ||x*_k||): X* stays feasible, the optimum is the same.
"""
import numpy as np

from oracle.cuadmm_oracle import OracleSolver
from tests._infeas_twin import Fixture, smat, svec

PROJ_ERR = 2e-12 * np.sqrt(2.0)          # kLbProjErr (csrc/lower_bound.h): the projection kernels' contract as their tests state it
LD = np.longdouble


def blk_lens(blk):
    return np.array([n * (n + 1) // 2 if n > 0 else -n for n in blk], np.int64)


class OptFixture(Fixture):
    pass


def make_opt_fixture(blk, m, seed):
    """Fixture (tests/_infeas_twin.py) with .Xs, .ys, .Ss, .pstar, .R (the trace bounds of the docstring)."""
    rng = np.random.default_rng(seed)
    lens = blk_lens(blk)
    off = np.concatenate([[0], np.cumsum(lens)])
    L = int(off[-1])
    Xs, Ss, R = np.zeros(L), np.zeros(L), np.zeros(len(blk))
    for k, n in enumerate(blk):
        sl = slice(off[k], off[k + 1])
        if n < 0:
            Xs[sl] = rng.standard_normal(-n)
            R[k] = 1.5 * np.linalg.norm(Xs[sl])
            continue
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        r = (k % 2) if n == 1 else max(1, n // 3)                   # rank of X*; blocks of size 1 alternate X* > 0 = S* and X* = 0 < S*
        d1, d2 = 0.5 + rng.random(r), 0.5 + rng.random(n - r)
        X = (Q[:, :r] * d1) @ Q[:, :r].T
        S = (Q[:, r:] * d2) @ Q[:, r:].T
        Xs[sl], Ss[sl] = svec((X + X.T) / 2), svec((S + S.T) / 2)
        R[k] = 1.5 * float(np.trace(X))
    A = rng.standard_normal((m, L)) / np.sqrt(L) * rng.uniform(0.5, 3.0, size=(m, 1))      # row norms from 0.5 to 3: normA is not all ones
    ys = rng.standard_normal(m)
    fx = OptFixture(blk, A, A @ Xs, A.T @ ys + Ss)
    fx.Xs, fx.ys, fx.Ss, fx.R = Xs, ys, Ss, R
    fx.pstar = float(np.sum((fx.b * ys).astype(LD)))
    return fx


def lower_bound(fx, y, R, proj_err=PROJ_ERR):
    """dict: lb, bty, penalty (floats of the longdouble sums), nu, nubar, norm_S (per block), worst (block of the largest term)"""
    Sh = fx.C - fx.A.T @ y
    off = fx.bidx.off
    nb = len(fx.blk)
    nu, nS, bar = np.zeros(nb), np.zeros(nb), np.zeros(nb)
    for k, n in enumerate(fx.blk):
        seg = Sh[off[k]:off[k + 1]]
        nS[k] = np.linalg.norm(seg)
        if n < 0:
            nu[k] = bar[k] = nS[k]
            continue
        w = np.linalg.eigvalsh(smat(-seg, int(n)))
        nu[k] = np.sqrt(np.sum(np.maximum(w, 0.0) ** 2))
        bar[k] = nu[k] + proj_err * np.sqrt(seg.size) * nS[k]
    R = np.asarray(R, np.float64)
    pen = np.sum(R.astype(LD) * bar.astype(LD))
    bty = np.sum(fx.b.astype(LD) * np.asarray(y, np.float64).astype(LD))
    return {"lb": float(bty - pen), "bty": float(bty), "penalty": float(pen), "nu": nu, "nubar": bar, "norm_S": nS,
            "worst": int(np.argmax(R * bar))}


def nu_tolerance(fx, norm_S):
    """per block: 2e-12 sqrt(len_k) ||S^_k||_F, twice the kernels' contract"""
    return 2e-12 * np.sqrt(blk_lens(fx.blk)) * norm_S


def form_error(fx, y):
    """per block: a bound on the rounding of S^ = C - A'y itself, which the bound does not cover: every entry is a sum
    of m + 1 products, formed by the engine in its scaled space (two more roundings per factor), so its error is at most
    (m + 8) 2^-53 (|C| + |A|'|y|) entrywise (Higham, Accuracy and Stability, (3.5)); the block's 2-norm of that.  It matters only where
    S^_k itself is at rounding level: an unconstrained block near the optimum."""
    e = (fx.m + 8) * 2.0 ** -53 * (np.abs(fx.C) + np.abs(fx.A).T @ np.abs(y))
    off = fx.bidx.off
    return np.array([np.linalg.norm(e[off[k]:off[k + 1]]) for k in range(len(fx.blk))])


def lb_tolerance(fx, tw, R):
    """sum_k R_k (2e-12 sqrt(len_k) ||S^_k||_F) + 64 2^-53 (|b'y| + sum_k R_k ||S^_k||)"""
    R = np.asarray(R, np.float64)
    lens = blk_lens(fx.blk)
    return float(np.sum(R * 2e-12 * np.sqrt(lens) * tw["norm_S"]) + 64 * 2.0 ** -53 * (abs(tw["bty"]) + np.sum(R * tw["norm_S"])))


def lb_sensitivity(fx, y, R):
    """|LB(y + d) - LB(y)| for |d_j| <= rel |y_j| is at most rel (|b|'|y| + sum_k R_k ||(|A|'|y|)_k||_2 (1 + PROJ_ERR sqrt(len_k))):
    P+ and the norms are 1-Lipschitz.  Returns the factor of rel."""
    e = np.abs(fx.A).T @ np.abs(y)
    off = fx.bidx.off
    n = np.array([np.linalg.norm(e[off[k]:off[k + 1]]) for k in range(len(fx.blk))])
    return float(np.abs(fx.b) @ np.abs(y) + np.sum(np.asarray(R) * n * (1 + PROJ_ERR * np.sqrt(blk_lens(fx.blk)))))


def gap(pobj, lb):
    return abs(pobj - lb) / (1 + abs(pobj) + abs(lb))


class Verdict(Exception):
    pass


class TwinResult:
    def __init__(self):
        self.status = 0
        self.iteration = 0
        self.checks = []              # (iteration, LB, g, errRp) of every check
        self.ys = []                  # y of every check, caller's units
        self.best = None              # (LB, iteration)
        self.y = None                 # y of the verdict, caller's units
        self.info = None


def twin_solve(fx, R, period, tol, max_iter, stop_tol, sig_update_threshold=500, sig_update_stage_1=50, sig_update_stage_2=100,
               switch_admm=11000, sigscale=1.05, sig=1.0):
    """The oracle on fx with the gap rule attached: status 5 and the verdict's iteration, or 1 / 2 as the solve ends."""
    o = OracleSolver().init_problem(fx.as_oracle_problem(), sig=sig)
    res = TwinResult()
    tol = tol if tol > 0 else stop_tol

    def hook(it, stage, **kw):
        if stage != "end" or period <= 0 or it % period != 0:
            return
        y = kw["y"] / o.normA * o.Cscale
        lb = lower_bound(fx, y, R)["lb"]
        g = gap(o.pobj, lb)
        res.checks.append((it, lb, g, o.errRp))
        res.ys.append(y)
        if res.best is None or lb > res.best[0]:
            res.best = (lb, it)
        if g <= tol and o.errRp <= tol:
            res.status, res.iteration, res.y = 5, it, y
            raise Verdict()

    try:
        o.solve(max_iter, stop_tol, sig_update_threshold, sig_update_stage_1, sig_update_stage_2, switch_admm, sigscale, stage_hook=hook)
        res.status = 1 if o.info.final_msg.endswith("converged.") else 2
        res.iteration = o.info.iter_num
    except Verdict:
        pass
    res.info = o.info
    return res
