"""np.longdouble twin of cuadmm_lowrank_line (include/cuadmm_amd.h; csrc/lowrank_line.h; DESIGN.md, "Line search along factor steps"), from
a fixture's dense A, b, C, blk.  With x(t) the resident X whose PSD blocks are (L_k + t D_k)(L_k + t D_k)':

    x0 = L L'   x1 = L D' + D L'   x2 = D D'   (PSD blocks; the free slices of x0 are X's, those of x1 and x2 zero)
    r0 = A x0 - b   p = A x1   q = A x2
    c0 = <C, x0> - y'r0 + (sigma / 2) r0'r0      c1 = <C, x1> - y'p + sigma r0'p      c2 = <C, x2> - y'q + (sigma / 2)(p'p + 2 r0'q)
    c3 = sigma p'q                               c4 = (sigma / 2) q'q

and the absolute-value chains the rounding contract is stated on (suffix "b"): the same formulas with every operand replaced by its
modulus and every sign by a plus,

    x0b = |L||L|'   x1b = |L||D|' + |D||L|'   x2b = |D||D|'   r0b = |A| x0b + |b|   pb = |A| x1b   qb = |A| x2b
    c0b = |C|.x0b + |y|.r0b + (sigma / 2) r0b.r0b   c1b = |C|.x1b + |y|.pb + sigma r0b.pb   c2b = |C|.x2b + |y|.qb + (sigma / 2)(pb.pb + 2 r0b.qb)
    c3b = sigma pb.qb   c4b = (sigma / 2) qb.qb

constants() counts the roundings of the engine's chain launch by launch, in the way of tests/_lowrank_grad_twin.py (u = 2^-53; c entries
in the fullest row of A, R the largest rank).  A slot of x0 or x2: the outer product's r_k + 4 and the factors' unit (6 behind a solve; else
A x takes fl(1 / bscale) and its product, 2): R + 10.  A slot of x1: 2 r_k + 4 and the same 6: 2 R + 10.
  r0       cuadmm_lowrank_grad's:                                                                   K_r = c + R + 16
  q        as r0 without b: inside                                                                  K_q = K_r
  p        A / normA 1, x1 2 R + 10, the product 1, at most c additions, the products by normA and bscale 2, two spare:
                                                                                                    K_p = c + 2 R + 16
  <C, x0>, <C, x2>   cuadmm_lowrank_grad's K_cx = vec_len + R + 16;   <C, x1>  K_cx1 = vec_len + 2 R + 16   (per block too)
  y'v      y 3, the scaled v at most K_v, the product 1, the sum's m + 264, bscale Cscale and its product 2:      K_v + m + 270
  v'w      K_v + K_w on a product, the product 1, the same sum, one spare:                                        K_v + K_w + m + 266
  c0       cuadmm_lowrank_grad's K_f = max(K_cx, K_r + m + 270, 2 K_r + m + 266) + 2
  c1       its three terms, the product by sigma and the two operations that join them:   max(K_cx1, K_p + m + 270, K_r + K_p + m + 266) + 3
  c2       the doubling is exact; the inner sum, the product by sigma / 2, two joins:     max(K_cx, K_q + m + 270, 2 K_p + m + 266, K_r + K_q + m + 266) + 4
  c3, c4   the product by sigma or sigma / 2 and one spare:                               K_p + K_q + m + 268,   2 K_q + m + 268
Every K is applied as gamma(K) = K u / (1 - K u).
"""
import numpy as np

from tests._block_mult_twin import LD, offsets
from tests._lowrank_grad_twin import gamma, svec_ld  # noqa: F401

U = 2.0 ** -53


def outer3(Lk, Dk):
    """svec of L L', L D' + D L', D D' in longdouble, and the chains of the three"""
    Lk, Dk = np.asarray(Lk, np.float64).astype(LD), np.asarray(Dk, np.float64).astype(LD)
    aL, aD = np.abs(Lk), np.abs(Dk)
    return ((svec_ld(Lk @ Lk.T), svec_ld(Lk @ Dk.T + Dk @ Lk.T), svec_ld(Dk @ Dk.T)),
            (svec_ld(aL @ aL.T), svec_ld(aL @ aD.T + aD @ aL.T), svec_ld(aD @ aD.T)))


def twin(fx, X, Ls, Ds, y, sigma):
    """dict of the exact quantities (longdouble) and their chains (suffix "b"): x (3 vectors), r, p, q, cx (3), per-block cx (nb, 3), c (5)"""
    blk = [int(n) for n in fx.blk]
    off = offsets(blk)
    A, b, C = fx.A.astype(LD), fx.b.astype(LD), fx.C.astype(LD)
    y = np.asarray(y, np.float64).astype(LD)
    sig = LD(sigma)
    X = np.asarray(X, np.float64).astype(LD)
    x = [X.copy(), np.zeros(X.size, LD), np.zeros(X.size, LD)]
    xb = [np.abs(X), np.zeros(X.size, LD), np.zeros(X.size, LD)]
    for k, n in enumerate(blk):
        if n > 0:
            v, vb = outer3(Ls[k], Ds[k])
            for j in range(3):
                x[j][off[k]:off[k + 1]] = v[j]
                xb[j][off[k]:off[k + 1]] = vb[j]
    aA, ab, aC, ay = np.abs(A), np.abs(b), np.abs(C), np.abs(y)
    r, p, q = A @ x[0] - b, A @ x[1], A @ x[2]
    rb, pb, qb = aA @ xb[0] + ab, aA @ xb[1], aA @ xb[2]
    cx, cxb = [np.sum(C * v) for v in x], [np.sum(aC * v) for v in xb]
    pbk = np.array([[np.sum((C * v)[off[k]:off[k + 1]]) for v in x] for k in range(len(blk))], LD)
    pbkb = np.array([[np.sum((aC * v)[off[k]:off[k + 1]]) for v in xb] for k in range(len(blk))], LD)
    c = [cx[0] - y @ r + sig / 2 * (r @ r), cx[1] - y @ p + sig * (r @ p), cx[2] - y @ q + sig / 2 * (p @ p + 2 * (r @ q)), sig * (p @ q), sig / 2 * (q @ q)]
    cb = [cxb[0] + ay @ rb + sig / 2 * (rb @ rb), cxb[1] + ay @ pb + sig * (rb @ pb), cxb[2] + ay @ qb + sig / 2 * (pb @ pb + 2 * (rb @ qb)), sig * (pb @ qb),
          sig / 2 * (qb @ qb)]
    return {"x": x, "xb": xb, "r": r, "rb": rb, "p": p, "pb": pb, "q": q, "qb": qb, "cx": cx, "cxb": cxb, "pbk": pbk, "pbkb": pbkb,
            "c": np.array(c, LD), "cb": np.array(cb, LD)}


def horner(c, t, dtype=np.float64):
    """c0 + c1 t + ... + c4 t^4 by Horner in dtype, as cuadmm_quartic_min evaluates a candidate"""
    c = [dtype(v) for v in c]
    t = dtype(t)
    return (((c[4] * t + c[3]) * t + c[2]) * t + c[1]) * t + c[0]


def horner_bar(cb, t):
    """sum |c_i| |t|^i in longdouble: what a rounding of a coefficient or of Horner's scheme is relative to"""
    return sum(LD(abs(v)) * abs(LD(t)) ** i for i, v in enumerate(cb))


def constants(fx, ranks):
    """the counted K of every output for this fixture and these ranks (module docstring)"""
    blk = [int(n) for n in fx.blk]
    c = int(np.max(np.count_nonzero(fx.A, axis=1)))
    R = max([int(r) for r, n in zip(ranks, blk) if n > 0] + [0])
    m = fx.m
    K = {"r": c + R + 16, "q": c + R + 16, "p": c + 2 * R + 16, "cx": fx.L + R + 16, "cx1": fx.L + 2 * R + 16}
    K["c0"] = max(K["cx"], K["r"] + m + 270, 2 * K["r"] + m + 266) + 2
    K["c1"] = max(K["cx1"], K["p"] + m + 270, K["r"] + K["p"] + m + 266) + 3
    K["c2"] = max(K["cx"], K["q"] + m + 270, 2 * K["p"] + m + 266, K["r"] + K["q"] + m + 266) + 4
    K["c3"] = K["p"] + K["q"] + m + 268
    K["c4"] = 2 * K["q"] + m + 268
    return K
