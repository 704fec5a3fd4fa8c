"""numpy twin of the infeasibility check (option "infeas_check": DESIGN.md, "Infeasibility certificates"; csrc/engine_reports.hip,
infeas_step) and the small problems its tests run on.

The twin is oracle.cuadmm_oracle.OracleSolver with a ``stage_hook`` at the end of every iteration: at iteration p it takes the
snapshot, at 2p, 3p, ... it forms the statistics of the check from y_k - y_{k-p}, X_k - X_{k-p} (the oracle's scaled iterates, the
same the engine holds) and applies the engine's rule, the dual test first.  A verdict ends the solve through an exception.

svec convention (oracle.BlockIndex): slot t of a block is entry (jj[t], ii[t]) with ii, jj = tril_indices(n), off-diagonal
entries times sqrt 2, so that dot products of svecs are trace inner products.
"""
import numpy as np

from oracle.cuadmm_oracle import BlockIndex, OracleSolver, Problem, coo_to_csc, psd_project_svec

SQRT2 = np.sqrt(2.0)
PROJ_ERR = 1e-12          # kInfeasProjErr (csrc/infeas.h)
STATUS = {0: "none", 1: "converged", 2: "iteration_limit", 3: "primal_infeasible", 4: "dual_infeasible"}


# ------------------------------------------------------------------------------------------------------------------------------
# problems
# ------------------------------------------------------------------------------------------------------------------------------
def svec(M):
    n = M.shape[0]
    ii, jj = np.tril_indices(n)
    return M[jj, ii] * np.where(ii == jj, 1.0, SQRT2)


def smat(v, n):
    ii, jj = np.tril_indices(n)
    M = np.zeros((n, n))
    w = v / np.where(ii == jj, 1.0, SQRT2)
    M[jj, ii] = w
    M[ii, jj] = w
    return M


def _E(n, i, j):
    M = np.zeros((n, n))
    M[i, j] += 0.5
    M[j, i] += 0.5
    return M


class Fixture:
    """Dense original data: A (m x L rows of svecs), b, C, blk; as_problem() gives the oracle's / the engine's Problem."""

    def __init__(self, blk, rows, b, C):
        self.blk = np.asarray(blk, np.int64)
        self.A = np.array(rows)
        self.b = np.asarray(b, np.float64)
        self.C = np.asarray(C, np.float64)
        self.m, self.L = self.A.shape
        self.bidx = BlockIndex(self.blk)

    def coo(self):
        r, c = np.nonzero(self.A.T)             # At: rows = svec slots, columns = constraints
        return r, c, self.A.T[r, c]

    def as_oracle_problem(self):
        r, c, v = self.coo()
        cp, rows, vals = coo_to_csc(c.copy(), r.copy(), v.copy(), self.m)
        bi = np.nonzero(self.b)[0]
        ci = np.nonzero(self.C)[0]
        return Problem(self.L, self.m, self.blk, cp, rows, vals, bi, self.b[bi], ci, self.C[ci])

    def with_b(self, b):
        return Fixture(self.blk, self.A, b, self.C)


def make_fixture(kind, big=False, seed=20261018):
    """kind: "P" (primal infeasible: X11 = X22 = 1, X12 = 2 in block 0), "F" (the same with X12 = 0.5: feasible), "D" (dual
    infeasible: X22 = X33 = 1, C0 = -E11, X11 free to grow).  big: blk = [3, 20, 70, -2] with feasible random constraints on the
    other PSD blocks and one constraint that touches the unconstrained block; else blk = [3, 4] with five on block 1."""
    rng = np.random.default_rng(seed)
    blk = [3, 20, 70, -2] if big else [3, 4]
    lens = [n * (n + 1) // 2 if n > 0 else -n for n in blk]
    off = np.concatenate([[0], np.cumsum(lens)])
    L = int(off[-1])
    rows, b = [], []

    def row(k, v):
        a = np.zeros(L)
        a[off[k]:off[k + 1]] = v
        return a

    if kind in ("P", "F"):
        rows += [row(0, svec(_E(3, 0, 0))), row(0, svec(_E(3, 1, 1))), row(0, svec(_E(3, 0, 1)))]
        b += [1.0, 1.0, 2.0 if kind == "P" else 0.5]
    else:
        rows += [row(0, svec(_E(3, 1, 1))), row(0, svec(_E(3, 2, 2)))]
        b += [1.0, 1.0]
    # feasible filler: random symmetric constraints, b from a random PSD point (and a point of the unconstrained block)
    Xhat = {}
    for k, n in enumerate(blk):
        if k == 0 or n < 0:
            continue
        G = rng.standard_normal((n, n)) / np.sqrt(n)
        Xhat[k] = svec(G @ G.T)
        for _ in range(5 if not big else (6 if n == 20 else 4)):
            M = rng.standard_normal((n, n))
            a = svec((M + M.T) / 2)
            rows.append(row(k, a))
            b.append(float(a @ Xhat[k]))
    if big:
        uhat = np.array([0.3, -0.7])
        M = rng.standard_normal((20, 20))
        a = row(1, svec((M + M.T) / 2))
        a[off[3]:off[4]] = [1.0, -1.0]
        rows.append(a)
        b.append(float(a[off[1]:off[2]] @ Xhat[1] + a[off[3]:off[4]] @ uhat))
    C = np.zeros(L)
    for k, n in enumerate(blk):
        if n > 0:
            C[off[k]:off[k + 1]] = svec(np.eye(n))
    if kind == "D":
        C[off[0]:off[1]] = svec(-1.0 * _E(3, 0, 0))           # _E(n, i, i) = E_ii
    return Fixture(blk, rows, b, C)


# ------------------------------------------------------------------------------------------------------------------------------
# the rule and the twin
# ------------------------------------------------------------------------------------------------------------------------------
def decide(stats, tol):
    """cuadmm_infeas_decide in numpy: (verdict, scalar, eta, radius)"""
    with np.errstate(all="ignore"):
        ny = np.sqrt(stats[0])
        if ny > 0 and np.isfinite(ny):
            beta, eta = stats[1] / ny, np.sqrt(stats[4]) / ny
            if beta > 0 and np.isfinite(beta) and eta >= 0 and eta <= tol * beta:
                return 3, beta, eta, (beta / eta if eta > 0 else np.inf)
        nx = np.sqrt(stats[2])
        if nx > 0 and np.isfinite(nx):
            gamma, e1, e2 = -stats[3] / nx, np.sqrt(stats[5]) / nx, np.sqrt(stats[6]) / nx
            eta = max(e1, e2)
            if gamma > 0 and np.isfinite(gamma) and e1 >= 0 and e2 >= 0 and eta <= tol * gamma:
                return 4, gamma, eta, (gamma / eta if eta > 0 else np.inf)
    return 0, 0.0, 0.0, 0.0


class Verdict(Exception):
    pass


class TwinResult:
    def __init__(self):
        self.status = 0
        self.iteration = 0
        self.checks = 0
        self.scalar = self.eta = self.radius = 0.0
        self.ray = None            # scaled space: dy (status 3) or dX (status 4)
        self.history = []          # (iteration, stats) of every check
        self.info = None
        self.y_cert = self.X_cert = None


def twin_solve(fx, period, tol, max_iter, stop_tol, sig_update_threshold=500, sig_update_stage_1=50, sig_update_stage_2=100,
               switch_admm=11000, sigscale=1.05, sig=1.0):
    """The oracle on fixture fx with the check attached.  Returns a TwinResult (status as cuadmm_get_status [0])."""
    o = OracleSolver().init_problem(fx.as_oracle_problem(), sig=sig)
    res = TwinResult()
    snap = {}
    nan = float("nan")

    def zero_free(v):
        v = v.copy()
        for lo, hi in o.bidx.free:
            v[lo:hi] = 0.0
        return v

    def hook(it, stage, **kw):
        if stage != "end" or period <= 0 or it % period != 0:
            return
        if max(o.maxfeas, o.relgap) < stop_tol:
            return
        X, y = kw["X"], kw["y"]
        if not snap:
            snap["X"], snap["y"] = X.copy(), y.copy()
            return
        dX, dy = X - snap["X"], y - snap["y"]
        snap["X"], snap["y"] = X.copy(), y.copy()
        res.checks += 1
        st = [float(dy @ dy), float(o.b @ dy), float(dX @ dX), float(o.C @ dX), nan, nan, nan, 0.0]
        verdict = (0, 0.0, 0.0, 0.0)
        if st[3] < 0 and st[2] > 0:              # the dual test first, as the engine runs them
            AdX = o.A @ dX
            pneg = zero_free(psd_project_svec(o.bidx, -dX))
            st[5], st[6] = float(AdX @ AdX), float(pneg @ pneg)
            verdict = decide([nan, nan, st[2], st[3], nan, st[5], st[6], 0.0], tol)
        if verdict[0] == 0 and st[1] > 0 and st[0] > 0:
            p = psd_project_svec(o.bidx, o.At_csr @ dy)
            st[4] = float(p @ p)
            verdict = decide([st[0], st[1], nan, nan, st[4], nan, nan, 0.0], tol)
        res.history.append((it, st))
        if verdict[0]:
            res.status, res.scalar, res.eta = verdict[0], verdict[1], verdict[2]
            # the engine's reported radius: scalar / (eta + eta_fl), eta_fl = 1e-12 sqrt(L) ||M||_F / ||d||
            M = o.At_csr @ dy
            eta_fl = PROJ_ERR * np.sqrt(X.size) * (np.sqrt(float(M @ M) / st[0]) if verdict[0] == 3 else 1.0)
            res.radius = verdict[1] / (verdict[2] + eta_fl) * (o.bscale if verdict[0] == 3 else o.Cscale)
            res.iteration = it
            res.ray = dy.copy() if verdict[0] == 3 else dX.copy()
            raise Verdict()

    try:
        o.solve(max_iter, stop_tol, sig_update_threshold, sig_update_stage_1, sig_update_stage_2, switch_admm, sigscale, stage_hook=hook)
        res.status = 1 if o.info.final_msg.endswith("converged.") else 2
        res.iteration = o.info.iter_num
    except Verdict:
        if res.status == 3:
            y = res.ray / o.normA
            res.y_cert = y / float(fx.b @ y)
        else:
            res.X_cert = res.ray / -float(fx.C @ res.ray)
    res.info = o.info
    return res


# ------------------------------------------------------------------------------------------------------------------------------
# verification of a certificate against the ORIGINAL data, without solver or twin
# ------------------------------------------------------------------------------------------------------------------------------
def psd_part_norm(fx, v, sign=1.0):
    """|| P+(sign v) ||_F over the PSD blocks (eigh per block), and the norm of v's slices of unconstrained blocks"""
    acc, free = 0.0, 0.0
    off = fx.bidx.off
    for k, n in enumerate(fx.blk):
        seg = v[off[k]:off[k + 1]]
        if n < 0:
            free += float(seg @ seg)
            continue
        w = np.linalg.eigvalsh(smat(sign * seg, int(n)))
        acc += float(np.sum(np.maximum(w, 0.0) ** 2))
    return np.sqrt(acc), np.sqrt(free)


def verify_primal(fx, y, radius):
    """(b'y - 1, ||P+(A'y)|| R with the unconstrained slices of A'y counted in full)"""
    Aty = fx.A.T @ y
    pn, fn = psd_part_norm(fx, Aty)
    viol = np.hypot(pn, fn)
    return float(fx.b @ y) - 1.0, (viol * radius if viol > 0 else 0.0)


def verify_dual(fx, X, radius):
    """(<C, X> + 1, max(||D^-1 A X||, ||P+(-X)||) R), D = diag(max(1, ||row of A||)); unconstrained slices carry no cone condition"""
    normA = np.maximum(1.0, np.linalg.norm(fx.A, axis=1))
    e1 = float(np.linalg.norm((fx.A @ X) / normA))
    e2, _ = psd_part_norm(fx, X, -1.0)
    viol = max(e1, e2)
    return float(fx.C @ X) + 1.0, (viol * radius if viol > 0 else 0.0)
