"""numpy twin of the accelerated iteration (option "accel": DESIGN.md, "Acceleration"; csrc/engine_iter.hip, accel_step).

Built on oracle.cuadmm_oracle.OracleSolver: its init, its scaling, _linsys and project.  ``accel_solve`` is OracleSolver.solve
statement for statement with the acceleration attached behind step 5; with accel = 0 it reproduces that method bit for bit
(tests/test_accel_host.py).  It is the reference of every trajectory comparison of tests/test_gpu_accel.py.

State u = (X, sig S).  Differences are formed as the kernels form them: g = (X - u_X, sig (S - u_S)).
"""
import numpy as np


class AccelLog:
    def __init__(self):
        self.taken = self.accepted = self.rejected = self.restarts = 0
        self.decisions = []          # (iteration that judged the candidate, "accept" / "reject")
        self.first_accept = None     # iteration (1-based) whose end accepted the first candidate
        self.cols = 0


def solve_ls(G, rhs, reg):
    """(G + reg tr(G) / cols I) gamma = rhs by Cholesky in longdouble; None when a pivot is not positive"""
    n = G.shape[0]
    M = G.astype(np.longdouble) + (np.longdouble(reg) * np.trace(G.astype(np.longdouble)) / n) * np.eye(n, dtype=np.longdouble)
    R = np.zeros((n, n), np.longdouble)
    for j in range(n):
        d = M[j, j] - np.dot(R[j, :j], R[j, :j])
        if not d > 0 or not np.isfinite(d):
            return None
        R[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            R[i, j] = (M[i, j] - np.dot(R[i, :j], R[j, :j])) / R[j, j]
    z = np.zeros(n, np.longdouble)
    for i in range(n):
        z[i] = (np.longdouble(rhs[i]) - np.dot(R[i, :i], z[:i])) / R[i, i]
    for i in range(n - 1, -1, -1):
        z[i] = (z[i] - np.dot(R[i + 1:, i], z[i + 1:])) / R[i, i]
    out = z.astype(np.float64)
    return out if np.all(np.isfinite(out)) else None


def accel_solve(o, max_iter, stop_tol, sig_update_threshold=500, sig_update_stage_1=50, sig_update_stage_2=100, switch_admm=11000,
                sigscale=1.05, accel=0, safeguard=2.0, reg=1e-10, gamma_perturb=0.0, stage_hook=None):
    """o: an initialised OracleSolver (if_first = True).  Returns (info, AccelLog).  gamma_perturb: every gamma_j is multiplied by
    1 + gamma_perturb cos(j) (the sensitivity runs behind the trajectory tolerances)."""
    sig_update_threshold = int(sig_update_threshold)
    info = o.info
    info.iter_num = 0
    breakyes = False
    A, At_csr = o.A, o.At_csr
    log = AccelLog()
    L = o.X.size

    # acceleration state
    dF, dG = [], []                     # columns, oldest first
    have_prev = False
    f_prev = g_prev = None
    u = np.concatenate([o.X, o.S]) if accel > 0 else None       # (X, S) the coming iteration starts from
    pending = None                      # fallback beside a candidate

    def clear():
        nonlocal have_prev, pending
        dF.clear(); dG.clear()
        have_prev = False
        pending = None

    X_best = y_best = S_best = None
    it = 1
    while it <= max_iter + 1:
        # Step 0
        if max(o.maxfeas, o.relgap) < stop_tol:
            breakyes = True
            info.final_msg = "Solver ended: converged."
        if it > max_iter:
            breakyes = True
            info.final_msg = "Solver ended: maximum iteration reached"
        if breakyes or (it <= 200 and it % 50 == 1) or (it > 200 and it % 100 == 1):
            info.log_rows.append((it - 1, o.errRp, o.errRd, o.pobj, o.dobj, o.relgap, o.sig))

        # Step 1
        rhsy = -(A @ o.SmC)
        rhsy += (1 / o.sig) * o.Rp
        o.y = o._linsys(rhsy)

        # Step 2
        o.Aty = At_csr @ o.y
        Rd1 = o.Aty - o.C
        Xb = o.X + Rd1 * o.sig
        if breakyes:
            if it > switch_admm and X_best is not None:
                o.X, o.y, o.S = X_best.copy(), y_best.copy(), S_best.copy()
            break
        Xproj = o.project(Xb, it)
        Xdiff = 1.0 * Xproj + (-1.0) * o.X
        o.S = (1 / o.sig) * Xdiff + (-1.0) * Rd1
        if stage_hook is not None:
            stage_hook(it, "proj", Xb=Xb, Xproj=Xproj, S=o.S)

        # Step 3
        o.SmC = o.S - o.C
        if it == switch_admm:
            sig_update_stage_2 = sig_update_stage_2 // 2
            sigscale = sigscale * 1.23
            o.best_KKT = max(o.maxfeas, o.relgap)
            X_best, y_best, S_best = o.X.copy(), o.y.copy(), o.S.copy()
        if it < switch_admm:
            rhsy = -(A @ o.SmC)
            rhsy += (1 / o.sig) * o.Rp
            o.y = o._linsys(rhsy)
            o.Aty = At_csr @ o.y
            Rd1 = o.Aty - o.C
        if it > switch_admm:
            if X_best is not None and pending is None and o.best_KKT > max(o.maxfeas, o.relgap):     # no snapshot of a candidate's iteration
                X_best, y_best, S_best = o.X.copy(), o.y.copy(), o.S.copy()
                o.best_KKT = max(o.maxfeas, o.relgap)

        # Step 4
        o.Rd = 1.0 * Rd1 + 1.0 * o.S
        tau = 1.95 if it < switch_admm else 1.618
        if o.errRd < stop_tol:
            tau = max(1.618, tau / 1.1)
        o.X = 1.0 * o.X + (tau * o.sig) * o.Rd

        # Step 5
        sig_of_iter = o.sig
        o.Rp = -(A @ o.X) + o.b
        o.errRp = float(np.linalg.norm(o.normA * o.Rp * o.bscale)) / o.norm_borg
        o.pobj = float(o.C @ o.X) * o.objscale
        o.errRd = float(np.linalg.norm(o.Rd * o.Cscale)) / o.norm_Corg
        o.dobj = float(o.b @ o.y) * o.objscale
        o.maxfeas = max(o.errRp, o.errRd)
        o.relgap = abs(o.pobj - o.dobj) / (1 + abs(o.pobj) + abs(o.dobj))
        feasratio = o.ratioconst * o.errRp / o.errRd
        if feasratio < 1:
            o.prim_win += 1
        else:
            o.dual_win += 1
        if ((it <= sig_update_threshold and it % sig_update_stage_1 == 1) or
                (it > sig_update_threshold and it % sig_update_stage_2 == 1)):
            if o.prim_win > 1.2 * o.dual_win:
                o.prim_win = 0
                o.sig = min(o.sigmax, o.sig * sigscale)
            elif o.dual_win > 1.2 * o.prim_win:
                o.dual_win = 0
                o.sig = max(o.sigmin, o.sig / sigscale)

        info.pobj.append(o.pobj); info.dobj.append(o.dobj)
        info.errRp.append(o.errRp); info.errRd.append(o.errRd)
        info.relgap.append(o.relgap); info.sig.append(o.sig)
        info.iter_num += 1
        if stage_hook is not None:
            stage_hook(it, "end", X=o.X, y=o.y, S=o.S)

        # ---- acceleration, behind the iteration (engine_iter.hip: accel_step)
        if accel > 0:
            nx = it + 1
            next_sig_may_change = ((nx <= sig_update_threshold and nx % sig_update_stage_1 == 1) or
                                   (nx > sig_update_threshold and nx % sig_update_stage_2 == 1))
            while True:                                   # one pass; "break" = the engine's "return"
                if o.sig != sig_of_iter:                  # the map changed in step 5
                    clear(); log.restarts += 1
                    u = np.concatenate([o.X, o.S])
                    break
                # push: g_k, the new columns, f_k
                f = np.concatenate([o.X, o.S])
                g = np.concatenate([o.X - u[:L], o.sig * (o.S - u[L:])])
                have_col = have_prev
                if have_col:
                    dF.append(np.concatenate([o.X - f_prev[:L], o.sig * (o.S - f_prev[L:])]))
                    dG.append(g - g_prev)
                    if len(dG) > accel:
                        dF.pop(0); dG.pop(0)
                gnorm2 = float(g @ g)
                if pending is not None:
                    fb = pending
                    pending = None
                    reject = (not safeguard > 0) or (not np.sqrt(gnorm2) <= safeguard * np.sqrt(fb["gnorm2"]))
                    if reject:
                        o.X, o.S, o.y, o.SmC, o.Rp = fb["X"], fb["S"], fb["y"], fb["SmC"], fb["Rp"]
                        (o.errRp, o.errRd, o.maxfeas, o.pobj, o.dobj, o.relgap, o.prim_win, o.dual_win) = fb["sc"]
                        clear()
                        u = np.concatenate([o.X, o.S])
                        log.rejected += 1
                        log.decisions.append((it, "reject"))
                        break
                    log.accepted += 1
                    log.decisions.append((it, "accept"))
                    if log.first_accept is None:
                        log.first_accept = it
                f_prev, g_prev, have_prev = f, g, True
                u = f
                tau_next = 1.95 if nx < switch_admm else 1.618
                if o.errRd < stop_tol:
                    tau_next = max(1.618, tau_next / 1.1)
                if tau_next != tau or nx == switch_admm:
                    clear(); log.restarts += 1
                    break
                if nx > max_iter or max(o.maxfeas, o.relgap) < stop_tol or next_sig_may_change or len(dG) < 2:
                    break
                Gm = np.array(dG)
                gamma = solve_ls(Gm @ Gm.T, Gm @ g, reg)
                if gamma is None:
                    clear(); log.restarts += 1
                    break
                if gamma_perturb:
                    gamma = gamma * (1 + gamma_perturb * np.cos(np.arange(gamma.size)))
                pending = {"X": o.X, "S": o.S, "y": o.y, "SmC": o.SmC, "Rp": o.Rp, "gnorm2": gnorm2,
                           "sc": (o.errRp, o.errRd, o.maxfeas, o.pobj, o.dobj, o.relgap, o.prim_win, o.dual_win)}
                Fm = np.array(dF)
                corr = gamma @ Fm
                o.X = o.X - corr[:L]
                o.S = (o.sig * o.S - corr[L:]) / o.sig
                u = np.concatenate([o.X, o.S])
                o.SmC = o.S - o.C                         # what a continued solve recomputes
                o.Rp = -(A @ o.X) + o.b
                log.taken += 1
                break
        it += 1

    o.X = o.X * o.bscale
    o.y = o.y / o.normA * o.Cscale
    o.S = o.S * o.Cscale
    log.cols = len(dG)
    return info, log
