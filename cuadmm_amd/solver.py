"""Host-side mirror of the reference's operator interface for the hot path.

``SDPSolver`` has the reference's method pair and member names (include/cuadmm/solver.h:30-248):
``init(...)`` / ``solve(...)`` with the same argument lists and defaults, then ``X``, ``y``, ``S``
(unscaled after solve), ``info_iter_num``, ``info_*_arr`` and ``total_time``.  ``Problem.from_txt``
mirrors Problem::from_txt (src/problem.cu:11-83).  Everything is executed by libcuadmm_amd.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

_INFO = {"pobj": 0, "dobj": 1, "errRp": 2, "errRd": 3, "relgap": 4, "sig": 5, "bscale": 6, "Cscale": 7}


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack_lowrank(blk_vals, Ls, who="set_lowrank"):
    """(L, ranks, rmax) as cuadmm_set_lowrank and cuadmm_block_multiply take them from a list of (n_k, r_k) arrays, one entry per block (those of unconstrained
    blocks are ignored): rmax = max(1, max r_k), block k at the prefix sum of n_j min(n_j, rmax) over the PSD blocks before it, column by
    column, the columns >= r_k zero.  ValueError on a wrong number of entries, a wrong row count or more columns than rows."""
    blk = [int(n) for n in blk_vals]
    if len(Ls) != len(blk):
        raise ValueError("%s: %d factors for %d blocks" % (who, len(Ls), len(blk)))
    ranks = np.zeros(len(blk), np.int32)
    mats = [None] * len(blk)
    for k, n in enumerate(blk):
        if n <= 0:
            continue
        A = _f64(Ls[k])
        if A.ndim != 2 or A.shape[0] != n or A.shape[1] > n:
            raise ValueError("%s: block %d has size %d, its factor the shape %s" % (who, k, n, A.shape))
        mats[k], ranks[k] = A, A.shape[1]
    rmax = max(1, int(ranks.max()) if ranks.size else 1)
    off = np.concatenate([[0], np.cumsum([n * min(n, rmax) if n > 0 else 0 for n in blk])]).astype(np.int64)
    L = np.zeros(max(int(off[-1]), 1))
    for k, A in enumerate(mats):
        if A is not None:
            L[off[k]:off[k] + A.size] = A.T.ravel()
    return L, ranks, rmax


def unpack_lowrank(blk_vals, ranks, rmax, buf):
    """the list of (n_k, r_k) arrays held by a buffer in the layout of pack_lowrank for this rmax ((0, 0) for unconstrained blocks)"""
    out, at = [], 0
    for k, n in enumerate(int(n) for n in blk_vals):
        r = int(ranks[k]) if n > 0 else 0
        out.append(buf[at:at + max(n, 0) * r].reshape(r, max(n, 0)).T.copy())
        at += n * min(n, rmax) if n > 0 else 0
    return out


def lowrank_grad_args(blk_vals, con_num, L, y, sigma):
    """(L buffer, ranks, rmax, y or None, sigma) as cuadmm_lowrank_grad takes them; ValueError on factors that do not fit the blocks, a y
    of another length than con_num, a sigma that is negative or not finite"""
    sigma = float(sigma)
    if not (sigma >= 0.0 and np.isfinite(sigma)):
        raise ValueError("lowrank_grad: sigma = %r, allowed is a finite sigma >= 0" % sigma)
    Lv, ranks, rmax = pack_lowrank(blk_vals, L, "lowrank_grad")
    if y is not None:
        y = _f64(y).ravel()
        if y.size != int(con_num):
            raise ValueError("lowrank_grad: y has %d entries, the problem %d" % (y.size, int(con_num)))
    return Lv, ranks, rmax, y, sigma


def lowrank_line_args(blk_vals, con_num, L, D, y, sigma, t_max):
    """(L buffer, D buffer, ranks, rmax, y or None, sigma, t_max) as cuadmm_lowrank_line takes them; ValueError where lowrank_grad_args
    raises one, on a D whose shapes are not those of L, and on a t_max that is not a number"""
    t_max = float(t_max)
    if np.isnan(t_max):
        raise ValueError("lowrank_line: t_max is not a number")
    sigma = float(sigma)
    if not (sigma >= 0.0 and np.isfinite(sigma)):
        raise ValueError("lowrank_line: sigma = %r, allowed is a finite sigma >= 0" % sigma)
    Lv, ranks, rmax = pack_lowrank(blk_vals, L, "lowrank_line")
    Dv, dranks, _ = pack_lowrank(blk_vals, D, "lowrank_line")
    if not np.array_equal(ranks, dranks):
        raise ValueError("lowrank_line: D has the ranks %s, L the ranks %s" % (dranks.tolist(), ranks.tolist()))
    if y is not None:
        y = _f64(y).ravel()
        if y.size != int(con_num):
            raise ValueError("lowrank_line: y has %d entries, the problem %d" % (y.size, int(con_num)))
    return Lv, Dv, ranks, rmax, y, sigma, t_max


def quartic_min(c, t_max):
    """The global minimiser of c[0] + c[1] t + ... + c[4] t^4 on [0, t_max] (cuadmm_quartic_min; no device is needed): a dict with "t",
    "f" = f(t), "decrease" = f(t) - c[0] and "critical", the number of interior critical points found.  t_max = inf where c[4] > 0, or
    c[4] = c[3] = 0 and c[2] > 0.  CuadmmError on coefficients that are not finite, a negative or NaN t_max, an unbounded problem."""
    c = _f64(c).ravel()
    if c.size != 5:
        raise ValueError("quartic_min: %d coefficients, expected 5" % c.size)
    o = np.zeros(4)
    check(_lib.load().cuadmm_quartic_min(_p(c), float(t_max), _p(o)))
    return {"t": float(o[0]), "f": float(o[1]), "decrease": float(o[2]), "critical": int(o[3])}


def cg_update(gg, go, gd, gg_prev, first):
    """The scalar step of lowrank_refine between a gradient and a direction (cuadmm_cg_update; no device is needed): from gg = <G, G>,
    go = <G, G_old>, gd = <G, D_old> and the gg of the step before, a dict with "beta" = max(0, (gg - go) / gg_prev) (0 where first or
    gg_prev == 0, and on a restart), "slope" = beta gd - gg and "restart" (first, or a slope that is not negative).  CuadmmError on an
    input that is not finite."""
    o = np.zeros(3)
    check(_lib.load().cuadmm_cg_update(float(gg), float(go), float(gd), float(gg_prev), int(bool(first)), _p(o)))
    return {"beta": float(o[0]), "slope": float(o[1]), "restart": bool(o[2])}


def lowrank_refine_args(blk_vals, con_num, L, y, sigma, steps, t_max, gtol):
    """(L buffer, ranks, rmax, y or None, sigma, steps, t_max, gtol) as cuadmm_lowrank_refine takes them; ValueError where
    lowrank_grad_args raises one, on steps < 1, a t_max that is not positive, a gtol that is negative or not finite"""
    sigma, t_max, gtol, steps = float(sigma), float(t_max), float(gtol), int(steps)
    if not (sigma >= 0.0 and np.isfinite(sigma)):
        raise ValueError("lowrank_refine: sigma = %r, allowed is a finite sigma >= 0" % sigma)
    if steps < 1:
        raise ValueError("lowrank_refine: steps = %d, allowed is steps >= 1" % steps)
    if not t_max > 0.0:
        raise ValueError("lowrank_refine: t_max = %r, allowed is t_max > 0" % t_max)
    if not (gtol >= 0.0 and np.isfinite(gtol)):
        raise ValueError("lowrank_refine: gtol = %r, allowed is a finite gtol >= 0" % gtol)
    Lv, ranks, rmax = pack_lowrank(blk_vals, L, "lowrank_refine")
    if y is not None:
        y = _f64(y).ravel()
        if y.size != int(con_num):
            raise ValueError("lowrank_refine: y has %d entries, the problem %d" % (y.size, int(con_num)))
    return Lv, ranks, rmax, y, sigma, steps, t_max, gtol


REFINE_TRACE = ("gg", "go", "gd", "beta", "slope", "restart", "c0", "c1", "c2", "c3", "c4", "t", "f", "ms")


class Problem:
    """TXT problem directory (blk.txt, con_num.txt, At.txt, b.txt, C.txt), src/problem.cu:11-83."""

    def __init__(self, vec_len, con_num, blk_vals, At_csc_col_ptrs, At_csc_row_ids, At_csc_vals,
                 b_indices, b_vals, C_indices, C_vals):
        self.vec_len, self.con_num = int(vec_len), int(con_num)
        self.blk_vals = _i32(blk_vals)
        self.mat_num = int(self.blk_vals.size)
        self.At_csc_col_ptrs, self.At_csc_row_ids = _i32(At_csc_col_ptrs), _i32(At_csc_row_ids)
        self.At_csc_vals = _f64(At_csc_vals)
        self.At_nnz = int(self.At_csc_vals.size)
        self.b_indices, self.b_vals = _i32(b_indices), _f64(b_vals)
        self.C_indices, self.C_vals = _i32(C_indices), _f64(C_vals)
        self.b_nnz, self.C_nnz = int(self.b_vals.size), int(self.C_vals.size)

    @classmethod
    def from_txt(cls, prefix):
        lib = _lib.load()
        h = C.c_void_p()
        check(lib.cuadmm_problem_from_txt(prefix.encode(), C.byref(h)))
        try:
            v = _lib.ProblemView()
            check(lib.cuadmm_problem_view_get(h, C.byref(v)))
            arr = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True) if n > 0 else np.zeros(0, dt)
            return cls(v.vec_len, v.con_num, arr(v.blk_vals, v.mat_num, np.int32),
                       arr(v.At_csc_col_ptrs, v.con_num + 1, np.int32), arr(v.At_csc_row_ids, v.At_nnz, np.int32),
                       arr(v.At_csc_vals, v.At_nnz, np.float64), arr(v.b_indices, v.b_nnz, np.int32),
                       arr(v.b_vals, v.b_nnz, np.float64), arr(v.C_indices, v.C_nnz, np.int32),
                       arr(v.C_vals, v.C_nnz, np.float64))
        finally:
            lib.cuadmm_problem_free(h)

    @classmethod
    def from_coo(cls, blk, con_num, At_row, At_col, At_val, b_idx, b_val, C_idx, C_val):
        """COO triplets of At (svec_row, constraint_col, value) -> sorted CSC (COO_to_CSC, io.cu:187-243)."""
        lib = _lib.load()
        blk = _i32(blk)
        b64 = blk.astype(np.int64)
        vec_len = int(np.sum(np.where(b64 >= 0, b64 * (b64 + 1) // 2, -b64)))     # negative size: unconstrained block
        rows, cols, vals = _i32(At_row).copy(), _i32(At_col).copy(), _f64(At_val).copy()
        cp = np.zeros(con_num + 1, np.int32)
        check(lib.cuadmm_coo_to_csc(_p(cp), _p(cols), _p(rows), _p(vals), int(vals.size), int(con_num)))
        return cls(vec_len, con_num, blk, cp, rows, vals, b_idx, b_val, C_idx, C_val)

    def trace_bounds(self):
        """Trace bounds read off the constraints (cuadmm_trace_bounds_detect): one number per block, -1 where nothing was found."""
        R = np.full(self.mat_num, -1.0)
        check(_lib.load().cuadmm_trace_bounds_detect(self.vec_len, self.con_num, _p(self.At_csc_col_ptrs), _p(self.At_csc_row_ids),
                                                     _p(self.At_csc_vals), _p(self.b_indices), _p(self.b_vals), self.b_nnz,
                                                     _p(self.blk_vals), self.mat_num, _p(R)))
        return R


class SDPSolver:
    """Mirror of class SDPSolver (include/cuadmm/solver.h:30-248)."""

    def __init__(self, device=0, verbose=True, rank=0, world=1, profile=False, force_comm=False, psd_steps=False,
                 eig_rank=0, eig_rank_begin_iter=0, eig_rank_maxfeas=0.0, options=None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        check(self._lib.cuadmm_create(C.byref(self._h)))
        for k, v in (("device", device), ("verbose", int(bool(verbose))), ("rank", rank), ("world", world),
                     ("profile", int(profile)), ("force_comm", int(bool(force_comm))), ("psd_steps", int(bool(psd_steps))),
                     ("eig_rank", int(eig_rank)), ("eig_rank_begin_iter", int(eig_rank_begin_iter)), ("eig_rank_maxfeas", float(eig_rank_maxfeas))):
            check(self._lib.cuadmm_set_option(self._h, k.encode(), float(v)))
        for k, v in (options or {}).items():           # engine options by name (include/cuadmm_amd.h: cuadmm_set_option)
            self.set_option(k, v)
        self._cb = None
        self.vec_len = self.con_num = 0

    def __del__(self):
        try:
            if self._h:
                self._lib.cuadmm_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_option(self, key, value):
        check(self._lib.cuadmm_set_option(self._h, key.encode(), float(value)))

    def counters(self):
        o = np.zeros(8)
        check(self._lib.cuadmm_get_counters(self._h, _p(o)))
        keys = ["batch_launches", "batch_iters", "batch_rollbacks", "host_pool_threads", "fused", "closed_blocks", "dev_solve", "tail_k"]
        return dict(zip(keys, o.tolist()))

    def group_info(self):
        """The in-process group this handle leads after duo_init(device_num_requested = N) from one process."""
        o = np.zeros(4)
        check(self._lib.cuadmm_get_group_info(self._h, _p(o)))
        return {"engines": int(o[0]), "exchange": "device" if o[1] else "host", "distinct_devices": int(o[2]), "allreduces": int(o[3])}

    def tail_info(self):
        """The dense GPU tail of the A A^T factor on this rank (cuadmm_get_tail_info)."""
        o = np.zeros(6)
        check(self._lib.cuadmm_get_tail_info(self._h, _p(o)))
        return {"tail_k": int(o[0]), "bytes_read_per_solve": float(o[1]), "rows": int(o[2]), "bytes_resident": float(o[3]),
                "inverse_residual": float(o[4]), "refined": bool(o[5])}

    def accel_info(self):
        """Option "accel" (cuadmm_get_accel_info): what the safeguarded Anderson acceleration did so far."""
        o = np.zeros(8)
        check(self._lib.cuadmm_get_accel_info(self._h, _p(o)))
        return {"memory": int(o[0]), "taken": int(o[1]), "accepted": int(o[2]), "rejected": int(o[3]), "restarts": int(o[4]),
                "columns": int(o[5]), "ms": float(o[6]), "ring_bytes": float(o[7])}

    STATUS_NAMES = ("none", "converged", "iteration_limit", "primal_infeasible", "dual_infeasible", "certified_gap")

    def status(self):
        """How the last solve ended (cuadmm_get_status); option "infeas_check" adds the two infeasible statuses, "gap_check" certified_gap."""
        o = np.zeros(8)
        check(self._lib.cuadmm_get_status(self._h, _p(o)))
        return {"status": int(o[0]), "name": self.STATUS_NAMES[int(o[0])], "iteration": int(o[1]), "checks": int(o[2]), "scalar": float(o[3]),
                "eta": float(o[4]), "radius": float(o[5]), "ms": float(o[6]), "bytes": float(o[7])}

    def certificate(self):
        """("primal", y) behind status primal_infeasible (b'y = 1), ("dual", X) behind dual_infeasible (<C, X> = -1)."""
        st = self.status()["status"]
        if st == 4:
            X = np.zeros(self.vec_len)
            check(self._lib.cuadmm_get_certificate(self._h, None, _p(X)))
            return "dual", X
        y = np.zeros(self.con_num)
        check(self._lib.cuadmm_get_certificate(self._h, _p(y), None))      # any status but 3: the library's error
        return "primal", y

    def set_trace_bounds(self, R):
        """One R_k >= 0 per block (PSD: tr X_k <= R_k, unconstrained: ||x_k|| <= R_k) for lower_bound() / option "gap_check"; None clears."""
        if R is None:
            check(self._lib.cuadmm_set_trace_bounds(self._h, None, 0))
            return
        Ra = _f64(R)
        check(self._lib.cuadmm_set_trace_bounds(self._h, _p(Ra), int(Ra.size)))

    def lower_bound(self, per_block=False):
        """The certified lower bound at the current y (cuadmm_lower_bound); per_block adds nu_k and ||S^_k||_F per block."""
        o = np.zeros(8)
        pb = np.zeros(2 * self.mat_num) if per_block else None
        check(self._lib.cuadmm_lower_bound(self._h, _p(o), _p(pb)))
        r = {"lower_bound": float(o[0]), "bty": float(o[1]), "penalty": float(o[2]), "gap": float(o[3]), "worst_block": int(o[4]),
             "worst_term": float(o[5]), "ms": float(o[6]), "bytes": float(o[7])}
        if per_block:
            r["nu"], r["norm_S"] = pb[0::2].copy(), pb[1::2].copy()
        return r

    def gap_info(self):
        """Option "gap_check" in the last solve (cuadmm_get_gap_info)."""
        o = np.zeros(8)
        check(self._lib.cuadmm_get_gap_info(self._h, _p(o)))
        return {"checks": int(o[0]), "best_lower_bound": float(o[1]), "best_iteration": int(o[2]), "last_lower_bound": float(o[3]),
                "last_gap": float(o[4]), "ms": float(o[5]), "bytes": float(o[6]), "verdict_iteration": int(o[7])}

    EVALUATE_KEYS = ("pobj", "dobj", "norm_Rp", "norm_Rd", "vX", "vS", "XS", "norm_b", "norm_C", "err1", "err2", "err3", "err4", "err5", "err6", "ms")

    def evaluate(self, X=None, y=None, S=None):
        """KKT and DIMACS report of a point in the caller's units (cuadmm_evaluate); None: the vector .X / .y / .S would return now.
        The named scalars of EVALUATE_KEYS and "per_block": (mat_num, 6) = ||X_k||, vX_k, ||S_k||, vS_k, <X_k, S_k>, ||Rd_k||."""
        Xa = None if X is None else _f64(X)
        ya = None if y is None else _f64(y)
        Sa = None if S is None else _f64(S)
        for a, n, what in ((Xa, self.vec_len, "X"), (ya, self.con_num, "y"), (Sa, self.vec_len, "S")):
            if a is not None and a.size != n:
                raise ValueError("evaluate: %s has %d entries, the problem %d" % (what, a.size, n))
        o = np.zeros(16)
        pb = np.zeros(6 * self.mat_num)
        check(self._lib.cuadmm_evaluate(self._h, _p(Xa), _p(ya), _p(Sa), _p(o), _p(pb)))
        r = dict(zip(self.EVALUATE_KEYS, o.tolist()))
        r["per_block"] = pb.reshape(self.mat_num, 6)
        return r

    def evaluate_info(self):
        """cuadmm_get_evaluate_info: calls so far, bytes the evaluation holds, bytes of the auxiliary projector, ms of the last call."""
        o = np.zeros(4)
        check(self._lib.cuadmm_get_evaluate_info(self._h, _p(o)))
        return {"calls": int(o[0]), "bytes": float(o[1]), "aux_bytes": float(o[2]), "ms": float(o[3])}

    LAMBDA_MIN_WHICH = {"X": 0, "S": 1, "dual": 2}

    def lambda_min(self, which="X", steps=12):
        """Certified lower bounds on lambda_min of every PSD block of X, S or ("dual") C - A'y at the current y (cuadmm_lambda_min).
        "lo" is certified, "hi" an estimate; "flag": 0 refined, 1 PSD at the floor, 2 unconstrained, 3 unrefined.  "lower_bound" is NaN
        unless which = "dual" and trace bounds are set."""
        if which not in self.LAMBDA_MIN_WHICH:
            raise ValueError("lambda_min: which must be 'X', 'S' or 'dual'")
        o = np.zeros(8)
        pb = np.zeros(3 * self.mat_num)
        check(self._lib.cuadmm_lambda_min(self._h, self.LAMBDA_MIN_WHICH[which], int(steps), _p(o), _p(pb)))
        return {"lambda_min": float(o[0]), "block": int(o[1]), "dimacs": float(o[2]), "lower_bound": float(o[3]), "unrefined": int(o[4]),
                "psd_at_floor": int(o[5]), "ms": float(o[6]), "bytes": float(o[7]), "lo": pb[0::3].copy(), "hi": pb[1::3].copy(),
                "flag": pb[2::3].astype(int)}

    LOWRANK_WHICH = {"X": 0, "S": 1}

    def lowrank(self, which="X", *, tol, rmax=None):
        """Numerical rank and a factor M_k ~ L_k L_k' of every PSD block of X or S by Cholesky with diagonal pivoting (cuadmm_lowrank), stopped
        where the largest residual diagonal entry is <= tol * max_i m_ii or at rmax columns (default: the largest block size).  Per block
        "rank", "resid", "dneg", "trace", "flag" (0 complete, 1 stopped at rmax, 2 unconstrained, 3 not factored); "L": a list of (n_k, r_k)
        arrays in the block's row order (unconstrained: (0, 0)); "piv": a list of the r_k pivot rows."""
        if which not in self.LOWRANK_WHICH:
            raise ValueError("lowrank: which must be 'X' or 'S'")
        blk = [int(n) for n in self.blk_vals]
        if rmax is None:
            rmax = max([n for n in blk if n > 0] + [1])
        rmax = int(rmax)
        count = C.c_longlong(0)
        check(self._lib.cuadmm_lowrank_size(self._h, rmax, C.byref(count)))
        o = np.zeros(8)
        pb = np.zeros(6 * self.mat_num)
        Lv = np.zeros(max(count.value, 1))
        pv = np.full(max(count.value, 1), -1, np.int32)
        check(self._lib.cuadmm_lowrank(self._h, self.LOWRANK_WHICH[which], float(tol), rmax, _p(o), _p(pb), _p(Lv), _p(pv)))
        pb = pb.reshape(-1, 6)
        rank, off = pb[:, 0].astype(int), pb[:, 5].astype(np.int64)
        L, piv = [], []
        for k, n in enumerate(blk):
            r = rank[k]
            L.append(Lv[off[k]:off[k] + max(n, 0) * r].reshape(r, max(n, 0)).T.copy())
            piv.append(pv[off[k]:off[k] + r].copy())
        return {"rank_sum": int(o[0]), "rank_max": int(o[1]), "block": int(o[2]), "resid_sum": float(o[3]), "dneg_min": float(o[4]), "capped": int(o[5]),
                "ms": float(o[6]), "bytes": float(o[7]), "rank": rank, "resid": pb[:, 1].copy(), "dneg": pb[:, 2].copy(), "trace": pb[:, 3].copy(),
                "flag": pb[:, 4].astype(int), "L": L, "piv": piv}

    def set_lowrank(self, X=None, S=None, sig=0.0):
        """Start the next solve from per-block factors (cuadmm_set_lowrank): X and / or S as the list of (n_k, r_k) arrays lowrank()["L"]
        returns, every PSD block becoming L_k L_k'.  Entries of unconstrained blocks are ignored, and those blocks, y and a matrix left
        None keep their values.  Returns {"X": ..., "S": ...} with "blocks", "rank_sum", "ms", "bytes_staged" for each matrix set."""
        out = {}
        for name, Ls in (("X", X), ("S", S)):
            if Ls is None:
                continue
            Lv, ranks, rmax = pack_lowrank(self.blk_vals, Ls)
            o = np.zeros(4)
            check(self._lib.cuadmm_set_lowrank(self._h, self.LOWRANK_WHICH[name], _p(Lv), _p(ranks), rmax, float(sig), _p(o)))
            out[name] = {"blocks": int(o[0]), "rank_sum": int(o[1]), "ms": float(o[2]), "bytes_staged": float(o[3])}
        return out

    def block_multiply(self, which, V):
        """W_k = M_k V_k for every PSD block of X, S or ("dual") C - A'y at the current y (cuadmm_block_multiply).  V: a list of (n_k, r_k)
        arrays, one entry per block, as lowrank()["L"] returns (entries of unconstrained blocks are ignored).  Returns "W": the list of
        (n_k, r_k) products ((0, 0) for unconstrained blocks); "per_block": (mat_num, 4) rows ||W_k||_F, <V_k, W_k>, ||V_k||_F, flag
        (0 multiplied, 2 unconstrained); "norm" = ||W||_F, "inner" = sum <V_k, W_k>, "block" / "block_norm": the block of the largest
        ||W_k||_F, "blocks", "rank_sum", "ms", "bytes".  Behind a solve the call leaves the pending scaled state as it is."""
        if which not in self.LAMBDA_MIN_WHICH:
            raise ValueError("block_multiply: which must be 'X', 'S' or 'dual'")
        Vv, ranks, rmax = pack_lowrank(self.blk_vals, V, "block_multiply")
        Wv = np.zeros(Vv.size)
        o = np.zeros(8)
        pb = np.zeros(4 * self.mat_num)
        check(self._lib.cuadmm_block_multiply(self._h, self.LAMBDA_MIN_WHICH[which], _p(Vv), _p(ranks), rmax, _p(Wv), _p(o), _p(pb)))
        W, at = [], 0
        for k, n in enumerate(int(n) for n in self.blk_vals):
            r = int(ranks[k])
            W.append(Wv[at:at + max(n, 0) * r].reshape(r, max(n, 0)).T.copy())
            at += n * min(n, rmax) if n > 0 else 0
        return {"W": W, "per_block": pb.reshape(self.mat_num, 4), "norm": float(o[0]), "inner": float(o[1]), "block": int(o[2]), "block_norm": float(o[3]),
                "blocks": int(o[4]), "rank_sum": int(o[5]), "ms": float(o[6]), "bytes": float(o[7])}

    def lowrank_grad(self, L, y=None, sigma=0.0, want_S=False):
        """Value and gradient of f = <C, x> - y'r + (sigma / 2) ||r||^2, r = A x - b, at the factors L (cuadmm_lowrank_grad): x is the
        resident X with every PSD block replaced by L_k L_k'.  L: a list of (n_k, r_k) arrays as lowrank()["L"] returns; y: con_num values
        or None for the resident y; sigma >= 0 in the caller's units.  Returns "G": the list of gradients 2 (C - A'(y - sigma r))_k L_k,
        shaped like L; "f", "cx" = <C, x>, "yr" = y'r, "rnorm" = ||r||, "r", "gnorm" = ||G||_F, "lg" = <L, G>, "ms", "bytes"; "per_block":
        (mat_num, 4) rows <C_k, x_k>, ||G_k||_F (unconstrained: ||S^_k||_F), <L_k, G_k>, ||L_k||_F^2; with want_S, "Shat": C - A'(y - sigma r)
        as a vector of vec_len.  The solver is left as it was: behind a solve the pending scaled state stays pending."""
        Lv, ranks, rmax, yv, sigma = lowrank_grad_args(self.blk_vals, self.con_num, L, y, sigma)
        Gv = np.zeros(Lv.size)
        r = np.zeros(max(self.con_num, 1))
        Sh = np.zeros(max(self.vec_len, 1)) if want_S else None
        o = np.zeros(8)
        pb = np.zeros(4 * self.mat_num)
        check(self._lib.cuadmm_lowrank_grad(self._h, _p(Lv), _p(ranks), rmax, _p(yv), sigma, _p(Gv), _p(r), _p(Sh), _p(o), _p(pb)))
        out = {"G": unpack_lowrank(self.blk_vals, ranks, rmax, Gv), "f": float(o[0]), "cx": float(o[1]), "yr": float(o[2]), "rnorm": float(o[3]),
               "r": r[:self.con_num], "gnorm": float(o[4]), "lg": float(o[5]), "ms": float(o[6]), "bytes": float(o[7]), "per_block": pb.reshape(self.mat_num, 4)}
        if want_S:
            out["Shat"] = Sh[:self.vec_len]
        return out

    def lowrank_line(self, L, D, y=None, sigma=0.0, t_max=float("inf")):
        """The exact quartic t -> f(L + t D) of lowrank_grad's f along the direction D, and its global minimiser on [0, t_max]
        (cuadmm_lowrank_line).  L, D: lists of (n_k, r_k) arrays of the same shapes, as lowrank()["L"] returns; y, sigma as in
        lowrank_grad.  Returns "coef": c0 .. c4; "t", "f" = f(t) by Horner, "decrease" = f(t) - c0, "critical" (t_max <= 0: coefficients
        only, t = 0); "r", "p", "q": r(t) = r + t p + t^2 q; "pnorm", "qnorm", "ms", "bytes"; "per_block": (mat_num, 4) rows <C_k, x0_k>,
        <C_k, x1_k>, <C_k, x2_k>, flag (0 PSD, 2 unconstrained).  t_max = inf needs a quartic that is bounded below (sigma > 0 and
        A (D D') != 0); otherwise CuadmmError.  The solver is left as it was: behind a solve the pending scaled state stays pending."""
        Lv, Dv, ranks, rmax, yv, sigma, t_max = lowrank_line_args(self.blk_vals, self.con_num, L, D, y, sigma, t_max)
        n = max(self.con_num, 1)
        coef, r, p, q, o, pb = np.zeros(5), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(8), np.zeros(4 * self.mat_num)
        check(self._lib.cuadmm_lowrank_line(self._h, _p(Lv), _p(Dv), _p(ranks), rmax, _p(yv), sigma, t_max, _p(coef), _p(r), _p(p), _p(q), _p(o), _p(pb)))
        m = self.con_num
        return {"coef": coef, "t": float(o[0]), "f": float(o[1]), "decrease": float(o[2]), "pnorm": float(o[3]), "qnorm": float(o[4]), "critical": int(o[5]),
                "ms": float(o[6]), "bytes": float(o[7]), "r": r[:m], "p": p[:m], "q": q[:m], "per_block": pb.reshape(self.mat_num, 4)}

    def lowrank_descent(self, L, y=None, sigma=1.0, steps=10, t_max=float("inf")):
        """An example that closes the loop of lowrank, lowrank_grad and lowrank_line: `steps` steps of Polak-Ribiere+ nonlinear conjugate
        gradients on f(L) = <C, x> - y'r + (sigma / 2) ||r||^2 over the factors of the PSD blocks, each one lowrank_grad call, one
        lowrank_line call (the exact minimiser of f along the direction on [0, t_max]) and L <- L + t D on the host.  The direction
        restarts to steepest descent where <G, D> >= 0.  The unconstrained slices of x stay at their resident values throughout: only the
        factors move.  Stops early where the line search returns t = 0.  Returns {"L": the final factors, "trace": one dict per step
        with "f", "gnorm", "t", "predicted" (the quartic's f(t)), "restart"}.  Not a tuned optimiser: no multiplier update, no rank
        adaptation."""
        Ls = [np.array(_f64(m), copy=True) for m in L]
        inner = lambda A, B: float(sum(np.sum(a * b) for a, b in zip(A, B)))
        trace, D, G_old = [], None, None
        for _ in range(int(steps)):
            g = self.lowrank_grad(Ls, y, sigma)
            G = g["G"]
            restart = D is None
            if not restart:
                gg = inner(G_old, G_old)
                beta = max(0.0, (inner(G, G) - inner(G, G_old)) / gg) if gg > 0 else 0.0
                D = [-a + beta * d for a, d in zip(G, D)]
                restart = inner(G, D) >= 0
            if restart:
                D = [-a for a in G]
            ln = self.lowrank_line(Ls, D, y, sigma, t_max)
            trace.append({"f": g["f"], "gnorm": g["gnorm"], "t": ln["t"], "predicted": ln["f"], "restart": bool(restart)})
            if ln["t"] == 0:
                break
            Ls = [a + ln["t"] * d for a, d in zip(Ls, D)]
            G_old = G
        return {"L": Ls, "trace": trace}

    def lowrank_refine(self, L, y=None, sigma=1.0, steps=10, t_max=float("inf"), gtol=0.0):
        """`steps` steps of Polak-Ribiere+ nonlinear conjugate gradients on lowrank_grad's f over the factors, with lowrank_line's exact
        line search, in one call: the factors, the direction and the gradients stay on the device and the host reads a few scalars per
        step (cuadmm_lowrank_refine; the recurrence of lowrank_descent without its per-step round trips).  L: a list of (n_k, r_k) arrays
        as lowrank()["L"] returns; y, sigma as in lowrank_grad, fixed for the call; gtol: stop where ||G||_F <= gtol (0: never).
        Returns "L": the refined factors, shaped like L; "trace": one dict per step begun with "gg", "go", "gd", "beta", "slope",
        "restart", "c0" .. "c4" ("c0" is f at the step's factors), "t", "f" = f(t), "ms"; "steps": steps taken; "reason": 0 all steps done,
        1 a step of t = 0, 2 gtol reached, 3 a sum or coefficient that is not finite, 4 a quartic that is not bounded below with t_max =
        inf (the last row of the trace is then the step that was not taken); "f0", "f", "gnorm", "ms", "bytes"; "r" = A x - b at the
        factors of the last step begun.  X is not changed (set_lowrank takes "L"); no multiplier update, no rank adaptation, no
        preconditioning.  The solver is left as it was: behind a solve the pending scaled state stays pending."""
        Lv, ranks, rmax, yv, sigma, steps, t_max, gtol = lowrank_refine_args(self.blk_vals, self.con_num, L, y, sigma, steps, t_max, gtol)
        Lo, tr, o, r = np.zeros(Lv.size), np.zeros(16 * steps), np.zeros(8), np.zeros(max(self.con_num, 1))
        check(self._lib.cuadmm_lowrank_refine(self._h, _p(Lv), _p(ranks), rmax, _p(yv), sigma, steps, t_max, gtol, _p(Lo), _p(tr), _p(o), _p(r)))
        taken, reason = int(o[0]), int(o[1])
        rows = tr.reshape(steps, 16)[:taken + (1 if reason else 0)]
        trace = [dict(zip(REFINE_TRACE, (float(v) for v in row[:14]))) for row in rows]
        for t in trace:
            t["restart"] = bool(t["restart"])
        return {"L": unpack_lowrank(self.blk_vals, ranks, rmax, Lo), "trace": trace, "steps": taken, "reason": reason, "f0": float(o[2]), "f": float(o[3]),
                "gnorm": float(o[4]), "ms": float(o[5]), "bytes": float(o[6]), "r": r[:self.con_num]}

    def set_allreduce(self, fn):
        """fn(dev_ptr:int, count:int, hip_stream:int) -> None : in-place sum over ranks on that stream."""
        def tramp(_user, buf, count, stream):
            try:
                fn(int(buf or 0), int(count), int(stream or 0))
                return 0
            except Exception as e:                     # surfaces as CUADMM_ERR_COMM
                import traceback
                traceback.print_exc()
                return 1
        self._cb = _lib.ALLREDUCE_FN(tramp)
        check(self._lib.cuadmm_set_allreduce(self._h, self._cb, None))

    # -- SDPSolver::init (solver.h:208-223) -------------------------------------------------
    def init(self, eig_stream_num_per_gpu, cpu_eig_thread_num, vec_len, con_num,
             At_csc_col_ptrs, At_csc_row_ids, At_csc_vals, At_nnz,
             b_indices, b_vals, b_nnz, C_indices, C_vals, C_nnz, blk_vals, mat_num,
             X=None, y=None, S=None, sig=1.0):
        a = [_i32(At_csc_col_ptrs), _i32(At_csc_row_ids), _f64(At_csc_vals), _i32(b_indices), _f64(b_vals),
             _i32(C_indices), _f64(C_vals), _i32(blk_vals)]
        Xa = None if X is None else _f64(X)
        ya = None if y is None else _f64(y)
        Sa = None if S is None else _f64(S)
        check(self._lib.cuadmm_init(self._h, int(eig_stream_num_per_gpu), int(cpu_eig_thread_num), int(vec_len),
                                    int(con_num), _p(a[0]), _p(a[1]), _p(a[2]), int(At_nnz), _p(a[3]), _p(a[4]),
                                    int(b_nnz), _p(a[5]), _p(a[6]), int(C_nnz), _p(a[7]), int(mat_num),
                                    _p(Xa), _p(ya), _p(Sa), float(sig)))
        self.vec_len, self.con_num, self.mat_num = int(vec_len), int(con_num), int(mat_num)
        self.blk_vals = a[7].copy()
        return self

    def init_problem(self, p, X=None, y=None, S=None, sig=1.0, eig_stream_num_per_gpu=15, cpu_eig_thread_num=30):
        return self.init(eig_stream_num_per_gpu, cpu_eig_thread_num, p.vec_len, p.con_num, p.At_csc_col_ptrs,
                         p.At_csc_row_ids, p.At_csc_vals, p.At_nnz, p.b_indices, p.b_vals, p.b_nnz,
                         p.C_indices, p.C_vals, p.C_nnz, p.blk_vals, p.mat_num, X, y, S, sig)

    # -- SDPSolver::solve (solver.h:236-244) ------------------------------------------------
    def solve(self, max_iter, stop_tol, sig_update_threshold=500, sig_update_stage_1=50, sig_update_stage_2=100,
              switch_admm=int(1.1e4), sigscale=1.05, if_first=True):
        check(self._lib.cuadmm_solve(self._h, int(max_iter), float(stop_tol), int(sig_update_threshold),
                                     int(sig_update_stage_1), int(sig_update_stage_2), int(switch_admm),
                                     float(sigscale), int(bool(if_first))))
        return self

    # -- SDPDuoSolver::init / ::solve (duo_solver.h:236-276): two block sizes only ---------------------
    def duo_init(self, if_gpu_eig_mom, device_num_requested, eig_stream_num_per_gpu, cpu_eig_thread_num, vec_len, con_num,
                 At_csc_col_ptrs, At_csc_row_ids, At_csc_vals, At_nnz, b_indices, b_vals, b_nnz,
                 C_indices, C_vals, C_nnz, blk_vals, mat_num, X=None, y=None, S=None, sig=2e2):
        a = [_i32(At_csc_col_ptrs), _i32(At_csc_row_ids), _f64(At_csc_vals), _i32(b_indices), _f64(b_vals),
             _i32(C_indices), _f64(C_vals), _i32(blk_vals)]
        Xa = None if X is None else _f64(X)
        ya = None if y is None else _f64(y)
        Sa = None if S is None else _f64(S)
        check(self._lib.cuadmm_duo_init(self._h, int(bool(if_gpu_eig_mom)), int(device_num_requested),
                                        int(eig_stream_num_per_gpu), int(cpu_eig_thread_num), int(vec_len), int(con_num),
                                        _p(a[0]), _p(a[1]), _p(a[2]), int(At_nnz), _p(a[3]), _p(a[4]), int(b_nnz),
                                        _p(a[5]), _p(a[6]), int(C_nnz), _p(a[7]), int(mat_num), _p(Xa), _p(ya), _p(Sa), float(sig)))
        self.vec_len, self.con_num, self.mat_num = int(vec_len), int(con_num), int(mat_num)
        self.blk_vals = a[7].copy()
        return self

    # -- results (public members of the reference class) -----------------------------------------
    def dims(self):
        """(vec_len, con_num, mat_num) in the caller's numbering (cuadmm_get_dims)."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.cuadmm_get_dims(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def shard(self):
        b, e, kb, ke = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        check(self._lib.cuadmm_get_shard(self._h, C.byref(b), C.byref(e), C.byref(kb), C.byref(ke)))
        return b.value, e.value, kb.value, ke.value

    def _vec(self, fn, n):
        out = np.empty(n, np.float64)
        check(fn(self._h, _p(out)))
        return out

    @property
    def X(self):
        b, e, _, _ = self.shard()
        return self._vec(self._lib.cuadmm_get_X, e - b)

    @property
    def S(self):
        b, e, _, _ = self.shard()
        return self._vec(self._lib.cuadmm_get_S, e - b)

    @property
    def y(self):
        return self._vec(self._lib.cuadmm_get_y, self.con_num)

    def set_XyS(self, X=None, y=None, S=None, sig=0.0):
        Xa = None if X is None else _f64(X)
        ya = None if y is None else _f64(y)
        Sa = None if S is None else _f64(S)
        check(self._lib.cuadmm_set_XyS(self._h, _p(Xa), _p(ya), _p(Sa), float(sig)))

    def update_bC(self, b_idx=None, b_val=None, C_idx=None, C_val=None, keep_iterate=True, sig=0.0):
        """New b and / or C (the caller's numbering and units, as in init) on the factored solver; None leaves that one unchanged.
        keep_iterate: the current X, y, S start the next solve (warm start), else zeros.  Nothing that depends on A is redone."""
        if (b_idx is None) != (b_val is None) or (C_idx is None) != (C_val is None):
            raise ValueError("update_bC: indices and values come together")
        bi, bv = (None, None) if b_idx is None else (_i32(b_idx), _f64(b_val))
        ci, cv = (None, None) if C_idx is None else (_i32(C_idx), _f64(C_val))
        if (bi is not None and bi.size != bv.size) or (ci is not None and ci.size != cv.size):
            raise ValueError("update_bC: as many indices as values")
        check(self._lib.cuadmm_update_bC(self._h, _p(bi), _p(bv), -1 if bi is None else int(bi.size),
                                         _p(ci), _p(cv), -1 if ci is None else int(ci.size), int(bool(keep_iterate)), float(sig)))
        return self

    def update_A(self, vals, keep_iterate=True, sig=0.0):
        """New values of A (At_csc_vals in the order given to init) on the sparsity pattern of init.  The ordering and the symbolic
        analysis are kept; factor, device matrices, y-solve data and scaling are formed again as init would (cuadmm_update_A)."""
        v = _f64(vals)
        check(self._lib.cuadmm_update_A(self._h, _p(v), int(v.size), int(bool(keep_iterate)), float(sig)))
        return self

    def update_info(self):
        """cuadmm_get_update_info: [updates so far, wall ms of the last one, host numeric factor ms, device part of the y-solve
        rebuild ms, orderings run on this handle, bytes that crossed to the device in the last update]"""
        o = np.zeros(6)
        check(self._lib.cuadmm_get_update_info(self._h, _p(o)))
        return o

    def update_pass_info(self):
        """cuadmm_get_update_pass_info (option profile = 1): [value pass ms, bytes, svec pass ms, bytes] of the last update_A"""
        o = np.zeros(4)
        check(self._lib.cuadmm_get_update_pass_info(self._h, _p(o)))
        return o

    @property
    def info_iter_num(self):
        return int(self._lib.cuadmm_get_info_iter_num(self._h))

    def info_arr(self, name):
        cap = 1 << 22
        n_total = 0
        out = np.empty(4096, np.float64)
        n = self._lib.cuadmm_get_info_array(self._h, _INFO[name], _p(out), out.size)
        if n == out.size:
            out = np.empty(cap, np.float64)
            n = self._lib.cuadmm_get_info_array(self._h, _INFO[name], _p(out), out.size)
        del n_total
        return out[:check(n)].copy()

    info_pobj_arr = property(lambda self: self.info_arr("pobj"))
    info_dobj_arr = property(lambda self: self.info_arr("dobj"))
    info_errRp_arr = property(lambda self: self.info_arr("errRp"))
    info_errRd_arr = property(lambda self: self.info_arr("errRd"))
    info_relgap_arr = property(lambda self: self.info_arr("relgap"))
    info_sig_arr = property(lambda self: self.info_arr("sig"))
    info_bscale_arr = property(lambda self: self.info_arr("bscale"))
    info_Cscale_arr = property(lambda self: self.info_arr("Cscale"))

    @property
    def total_time(self):
        return float(self._lib.cuadmm_get_total_time(self._h))

    def state(self):
        o = np.zeros(12)
        check(self._lib.cuadmm_get_state(self._h, _p(o)))
        keys = ["errRp", "errRd", "pobj", "dobj", "relgap", "sig", "bscale", "Cscale", "norm_borg", "norm_Corg",
                "best_KKT", "eig_not_converged"]
        return dict(zip(keys, o.tolist()))

    def profile(self):
        o = np.zeros(24)
        check(self._lib.cuadmm_get_profile(self._h, _p(o)))
        names = ["aty_xb", "psd_project", "post_proj", "spmv_A", "copies", "host", "allreduce", "tail_solve"]
        return {n: dict(launches=o[3 * i], ms=o[3 * i + 1], bytes_per_launch=o[3 * i + 2]) for i, n in enumerate(names)}

    def psd_steps(self):
        """Newton-Schulz steps of the last projection per local block (needs psd_steps=True at construction)."""
        b, e, kb, ke = self.shard()
        out = np.zeros(max(ke - kb, 1), np.int32)
        n = self._lib.cuadmm_get_psd_steps(self._h, _p(out), out.size)
        check(min(n, 0))
        return out[:n]

    def reset_profile(self):
        check(self._lib.cuadmm_reset_profile(self._h))
