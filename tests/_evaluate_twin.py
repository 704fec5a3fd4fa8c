"""numpy twin of cuadmm_evaluate (include/cuadmm_amd.h; DESIGN.md, "Evaluation of a point"): the KKT and DIMACS report of a point
(X, y, S) from the ORIGINAL A, b, C of a fixture (tests/_infeas_twin.py: Fixture; tests/_lower_bound_twin.py: make_opt_fixture), in
the caller's units.  Sums and products run in np.longdouble; P+ is numpy.linalg.eigh per block (float64: the eigensolver's own
error, a few n 2^-53 ||M||, is far below every tolerance that uses it).

    per_block[k] = ||X_k||, vX_k = ||P+(-X_k)||_F, ||S_k||, vS_k = ||P+(-S_k)||_F, <X_k, S_k>, ||Rd_k||,   Rd = A'y + S - C
    out16        = pobj, dobj, ||A X - b||, ||Rd||, vX, vS, <X, S>, ||b||, ||C||, err1 .. err6, 0

An unconstrained block: vX_k = 0, vS_k = ||S_k||.  evaluate() also returns the absolute sums and the entrywise bounds the tests'
tolerances are made of.
"""
import numpy as np

from tests._infeas_twin import smat
from tests._lower_bound_twin import blk_lens

LD = np.longdouble
U = 2.0 ** -53
KEYS = ("pobj", "dobj", "norm_Rp", "norm_Rd", "vX", "vS", "XS", "norm_b", "norm_C", "err1", "err2", "err3", "err4", "err5", "err6", "ms")


def neg_part_norm(seg, n):
    """||P+(-M)||_F of the block svec `seg`: the 2-norm of the negative eigenvalues of M"""
    w = np.linalg.eigh(smat(np.asarray(seg, np.float64), int(n)))[0]
    return float(np.sqrt(np.sum(np.minimum(w, 0.0).astype(LD) ** 2)))


def _norm(v):
    return float(np.sqrt(np.sum(np.asarray(v, LD) ** 2)))


def evaluate(fx, X, y, S):
    """dict: out (16), per_block (mat_num, 6), and for the tolerances abs_XS (per block: sum |X_i S_i|), abs_cx, abs_by,
    rp_bound = ||(row length + 8) 2^-53 (|A||X| + |b|)||, rd_bound (per block) = ||(column length + 8) 2^-53 (|C| + |A|'|y| + |S|)||_k"""
    A, b, C = fx.A.astype(LD), fx.b.astype(LD), fx.C.astype(LD)
    X, y, S = np.asarray(X, np.float64), np.asarray(y, np.float64), np.asarray(S, np.float64)
    Xl, yl, Sl = X.astype(LD), y.astype(LD), S.astype(LD)
    off = np.concatenate([[0], np.cumsum(blk_lens(fx.blk))])
    nb = len(fx.blk)
    Rp = A @ Xl - b
    Rd = A.T @ yl + Sl - C
    pb = np.zeros((nb, 6))
    abs_XS = np.zeros(nb)
    for k, n in enumerate(fx.blk):
        sl = slice(off[k], off[k + 1])
        pb[k, 0], pb[k, 2] = _norm(Xl[sl]), _norm(Sl[sl])
        if n < 0:
            pb[k, 1], pb[k, 3] = 0.0, pb[k, 2]
        else:
            pb[k, 1], pb[k, 3] = neg_part_norm(X[sl], n), neg_part_norm(S[sl], n)
        pb[k, 4] = float(np.sum(Xl[sl] * Sl[sl]))
        abs_XS[k] = float(np.sum(np.abs(Xl[sl] * Sl[sl])))
        pb[k, 5] = _norm(Rd[sl])
    o = np.zeros(16)
    o[0], o[1] = float(np.sum(C * Xl)), float(np.sum(b * yl))
    o[2], o[3] = _norm(Rp), _norm(Rd)
    o[4], o[5] = _norm(pb[:, 1]), _norm(pb[:, 3])
    o[6] = float(np.sum(Xl * Sl))
    o[7], o[8] = _norm(b), _norm(C)
    den = 1 + abs(o[0]) + abs(o[1])
    o[9], o[10], o[11], o[12] = o[2] / (1 + o[7]), o[4] / (1 + o[7]), o[3] / (1 + o[8]), o[5] / (1 + o[8])
    o[13], o[14] = (o[0] - o[1]) / den, o[6] / den
    rowlen = np.count_nonzero(fx.A, axis=1)
    collen = np.count_nonzero(fx.A, axis=0)
    e_rp = (rowlen + 8) * U * (np.abs(fx.A) @ np.abs(X) + np.abs(fx.b))
    e_rd = (collen + 8) * U * (np.abs(fx.C) + np.abs(fx.A).T @ np.abs(y) + np.abs(S))
    return {"out": o, "per_block": pb, "abs_XS": abs_XS, "abs_cx": float(np.sum(np.abs(C * Xl))), "abs_by": float(np.sum(np.abs(b * yl))),
            "rp_bound": float(np.linalg.norm(e_rp)), "rd_bound": np.array([np.linalg.norm(e_rd[off[k]:off[k + 1]]) for k in range(nb)]),
            **dict(zip(KEYS, o.tolist()))}
