"""np.longdouble twin of cuadmm_lowrank_grad (include/cuadmm_amd.h; csrc/lowrank_grad.h; DESIGN.md, "Value and gradient at factors"), from a
fixture's dense A, b, C, blk:

    x = X with every PSD block k replaced by L_k L_k'      r = A x - b      f = <C, x> - y'r + (sigma / 2) ||r||^2
    ytilde = y - sigma r      S^ = C - A'ytilde      G_k = 2 S^_k L_k

and the absolute-value chains the rounding contract is stated on: the same formulas with every operand replaced by its modulus,

    xbar = sum |L||L| (PSD), |X| (free)   rbar = |A| xbar + |b|   ybar = |y| + sigma rbar   Sbar = |C| + |A'| ybar   Gbar = 2 Sbar |L|
    fbar = |C|.xbar + |y|.rbar + (sigma / 2) rbar.rbar

constants() counts the roundings of the engine's chain, launch by launch (u = 2^-53; c_i entries in row i of A, c'_i in row i of A', R the
largest rank, n the largest PSD block).  The factor of a slot of x: the outer product's contract r_k + 4; behind a solve the factors are
staged times fl(1 / sqrt(bscale)) (sqrt, division, product: 3 per factor, 6 per product of two), else A x takes fl(1 / bscale) and its
product (2): R + 10.
  r_i      A / normA 1, x R + 10, the product 1, at most c_i additions, the subtraction of b 1, the products by normA and bscale 2
           (on b: / normA, fl(1 / bscale) and its product, and the same three: 6):                         K_r = c + R + 16, one spare
  ytilde   y scaled 3 (normA, fl(1 / Cscale), its product); sigma r scaled: r, three products, fl(1 / Cscale);
           the subtraction 1:                                                                              K_y = K_r + 5
  S^_i     A / normA 1, ytilde K_y, the product 1, at most c'_i additions (C's among them), the unit Cscale 1
           (on C: 4, as in test_dual_matrix_against_longdouble):                                           K_S = c' + K_r + 8
  G        the block product's n + 4 on the matrix that was formed, one spare for the second-order term; the doubling is exact:
                                                                                                           K_G = K_S + n + 5
  <C, x>   C / Cscale 2, x R + 10, the product 1, at most vec_len additions in any order, the unit's product and its own 2:
                                                                                                           K_cx = vec_len + R + 16
  y'r      y 3, the scaled residual at most K_r, the product 1, the sum (a thread's terms, the workgroup's tree, 256 slots on the
           host: at most m + 264 additions on a term's path), bscale Cscale and its product 2:              K_yr = K_r + m + 270
  (sigma / 2) ||r||^2   r_i^2 2 K_r + 1, the same sum, the product by sigma / 2 1:                          K_rr = 2 K_r + m + 266
  f        the largest of the three and the two operations that join them:                                 K_f = max(...) + 2
Every K is applied as gamma(K) = K u / (1 - K u).
"""
import numpy as np

from tests._block_mult_twin import LD, U, matrix, offsets

SQ2 = np.sqrt(LD(2))


def svec_ld(M):
    """svec of a symmetric longdouble matrix: the lower triangle row by row, off-diagonal entries times sqrt(2)"""
    n = M.shape[0]
    ii, jj = np.tril_indices(n)
    return M[ii, jj] * np.where(ii == jj, LD(1), SQ2)


def gamma(K):
    K = np.asarray(K).astype(LD)
    return K * LD(U) / (1 - K * LD(U))


def twin(fx, X, Ls, y, sigma):
    """dict of the exact quantities (longdouble) and their chains (suffix "b"); G / Gb: lists of (n_k, r_k) arrays, (0, 0) for free blocks"""
    blk = [int(n) for n in fx.blk]
    off = offsets(blk)
    A, b, C = fx.A.astype(LD), fx.b.astype(LD), fx.C.astype(LD)
    y = np.asarray(y, np.float64).astype(LD)
    sig = LD(sigma)
    x, xb = np.asarray(X, np.float64).astype(LD).copy(), np.abs(np.asarray(X, np.float64).astype(LD))
    for k, n in enumerate(blk):
        if n > 0:
            Lk = np.asarray(Ls[k], np.float64).astype(LD)
            x[off[k]:off[k + 1]] = svec_ld(Lk @ Lk.T)
            xb[off[k]:off[k + 1]] = svec_ld(np.abs(Lk) @ np.abs(Lk).T)
    r, rb = A @ x - b, np.abs(A) @ xb + np.abs(b)
    cx, yr, rr = np.sum(C * x), np.sum(y * r), np.sum(r * r)
    f = cx - yr + sig / 2 * rr
    fb = np.sum(np.abs(C) * xb) + np.sum(np.abs(y) * rb) + sig / 2 * np.sum(rb * rb)
    yt, yb = y - sig * r, np.abs(y) + sig * rb
    Sh, Sb = C - A.T @ yt, np.abs(C) + np.abs(A).T @ yb
    G, Gb = [], []
    for k, n in enumerate(blk):
        if n <= 0:
            G.append(np.zeros((0, 0), LD))
            Gb.append(np.zeros((0, 0), LD))
            continue
        Lk = np.asarray(Ls[k], np.float64).astype(LD)
        G.append(2 * (matrix(Sh[off[k]:off[k + 1]], n) @ Lk))
        Gb.append(2 * (matrix(Sb[off[k]:off[k + 1]], n) @ np.abs(Lk)))
    return {"x": x, "xb": xb, "r": r, "rb": rb, "cx": cx, "cxb": np.sum(np.abs(C) * xb), "yr": yr, "yrb": np.sum(np.abs(y) * rb), "rr": rr,
            "rrb": np.sum(rb * rb), "f": f, "fb": fb, "yt": yt, "yb": yb, "Sh": Sh, "Sb": Sb, "G": G, "Gb": Gb}


def inner(Gs, Ds):
    """sum_k <G_k, D_k> in longdouble"""
    return sum((np.sum(np.asarray(g).astype(LD) * np.asarray(d).astype(LD)) for g, d in zip(Gs, Ds)), LD(0))


def five_point(fs, h):
    """(f(-2h) - 8 f(-h) + 8 f(h) - f(2h)) / (12 h) from fs = [f(-2h), f(-h), f(h), f(2h)]: the derivative at 0 of a quartic, exactly"""
    fs = [LD(v) for v in fs]
    return (fs[0] - 8 * fs[1] + 8 * fs[2] - fs[3]) / (12 * LD(h))


def constants(fx, ranks):
    """the counted K of every output for this fixture and these ranks (module docstring)"""
    blk = [int(n) for n in fx.blk]
    c = int(np.max(np.count_nonzero(fx.A, axis=1)))
    ct = int(np.max(np.count_nonzero(fx.A, axis=0)))
    R = max([int(r) for r, n in zip(ranks, blk) if n > 0] + [0])
    n = max([n for n in blk if n > 0] + [1])
    K = {"r": c + R + 16}
    K["y"] = K["r"] + 5
    K["S"] = ct + K["r"] + 8
    K["G"] = K["S"] + n + 5
    K["cx"] = fx.L + R + 16
    K["yr"] = K["r"] + fx.m + 270
    K["rr"] = 2 * K["r"] + fx.m + 266
    K["f"] = max(K["cx"], K["yr"], K["rr"]) + 2
    return K
