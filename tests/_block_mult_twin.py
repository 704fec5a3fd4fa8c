"""numpy twins of the block product W_k = M_k V_k on svec blocks (include/cuadmm_amd.h: cuadmm_block_multiply, cuadmm_op_block_mult;
csrc/block_mult.h; DESIGN.md, "Blocks times factors") and the packing of its buffers.

With s_ij the raw svec slot of (i, j) the kernel forms W[i, t] = sign * fma(K, sum_{j != i} s_ij V[j, t], s_ii V[i, t]), K = kInvSqrt2.
Two references:

  reference(seg, n, V, sign)  np.longdouble: sign * M V with M_ij = s_ij / sqrt(2) (i != j), s_ii, and A = |M| |V|, the sum the rounding
                              contract |W - exact| <= (n + 4) u A is stated on.  Its own error, (n + 2) 2^-64 A, is far inside the spare u.
  exact(seg, n, V, sign)      small-integer slots and V: the sum is an integer, so the result is sign * RN(K * offd + s_ii V_it), an exact
                              rational rounded once; float(Fraction) rounds correctly.

host_sums reproduces per_block and out8[0:6] of cuadmm_block_multiply from W and V: products rounded, then added, in index order (a
cumulative sum in numpy is that sequential sum).
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
K = 0.7071067811865476                       # kInvSqrt2 (csrc/block_mult.h)


def blk_lens(blk):
    return np.array([n * (n + 1) // 2 if n > 0 else -n for n in blk], np.int64)


def offsets(blk):
    return np.concatenate([[0], np.cumsum(blk_lens(blk))]).astype(np.int64)


def lowrank_size(blk, rmax):
    return int(sum(n * min(n, rmax) for n in blk if n > 0))


def loffs(blk, rmax):
    return np.concatenate([[0], np.cumsum([n * min(n, rmax) if n > 0 else 0 for n in blk])]).astype(np.int64)


def raw_smat(seg, n, dtype=np.float64):
    """the symmetric matrix of the raw slots: entry (i, j) = seg[max (max + 1) / 2 + min], nothing scaled"""
    M = np.zeros((n, n), dtype)
    ii, jj = np.tril_indices(n)
    M[ii, jj] = seg
    M[jj, ii] = seg
    return M


def matrix(seg, n):
    """the matrix the block stands for, in longdouble: off-diagonal slots / sqrt(2)"""
    M = raw_smat(np.asarray(seg).astype(LD), n, LD)
    d = np.diag(M).copy()
    M = M / np.sqrt(LD(2))
    M[np.diag_indices(n)] = d
    return M


def reference(seg, n, V, sign=1.0):
    """(sign * M V, |M| |V|) in longdouble"""
    M = matrix(seg, n)
    Vl = np.asarray(V).astype(LD)
    return LD(sign) * (M @ Vl), np.abs(M) @ np.abs(Vl)


def exact(seg, n, V, sign=1.0):
    """small-integer slots and V: float64 array of sign * RN(K * offd + s_ii V_it)"""
    S = raw_smat(np.asarray(seg), n).astype(np.int64)
    Vi = np.asarray(V).astype(np.int64)
    assert np.array_equal(S, raw_smat(np.asarray(seg), n)) and np.array_equal(Vi, np.asarray(V))
    d = np.diag(S).copy()
    S[np.diag_indices(n)] = 0
    offd = S @ Vi
    diag = d[:, None] * Vi
    k = Fraction(K)
    out = np.empty(Vi.shape)
    for i in range(Vi.shape[0]):
        for t in range(Vi.shape[1]):
            out[i, t] = sign * float(k * int(offd[i, t]) + int(diag[i, t]))
    return out


def pack(blk, Vs, rmax, fill=np.nan):
    """(buffer, ranks): the V buffer for rmax with `fill` in every column that must not be read; the ranks of unconstrained blocks are junk"""
    buf = np.full(max(lowrank_size(blk, rmax), 1), fill)
    ranks = np.zeros(len(blk), np.int32)
    lo = loffs(blk, rmax)
    for k, n in enumerate(blk):
        if n <= 0:
            ranks[k] = 77
            continue
        r = Vs[k].shape[1]
        assert Vs[k].shape[0] == n and r <= min(n, rmax)
        buf[lo[k]:lo[k] + n * r] = np.asarray(Vs[k], np.float64).T.ravel()
        ranks[k] = r
    return buf, ranks


def unpack(blk, ranks, rmax, buf):
    """(list of (n_k, r_k) arrays, list of the entries behind them in the block's range); (0, 0) and empty for unconstrained blocks"""
    lo = loffs(blk, rmax)
    Ws, pads = [], []
    for k, n in enumerate(blk):
        if n <= 0:
            Ws.append(np.zeros((0, 0)))
            pads.append(np.zeros(0))
            continue
        r = int(ranks[k])
        Ws.append(buf[lo[k]:lo[k] + n * r].reshape(r, n).T.copy())
        pads.append(buf[lo[k] + n * r:lo[k + 1]].copy())
    return Ws, pads


def seq_dot(a, b):
    """q = 0; q = q + a[e] * b[e] in index order, every product and sum rounded to double"""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    return float(np.cumsum(p)[-1]) + 0.0 if p.size else 0.0          # (+ 0.0: the sum starts from + 0.0, so it never ends at - 0.0)


def host_sums(blk, Vs, Ws):
    """(per_block (mat_num, 4), out6) as cuadmm_block_multiply forms them from the returned W and the caller's V"""
    pb = np.zeros((len(blk), 4))
    sq_all = dot_all = best = 0.0
    arg, blocks, rank_sum = -1, 0, 0
    for k, n in enumerate(blk):
        if n <= 0:
            pb[k, 3] = 2.0
            continue
        w, v = Ws[k].T.ravel(), np.asarray(Vs[k], np.float64).T.ravel()
        sq, dot, vsq = seq_dot(w, w), seq_dot(v, w), seq_dot(v, v)
        pb[k, :3] = np.sqrt(sq), dot, np.sqrt(vsq)
        sq_all, dot_all = sq_all + sq, dot_all + dot
        blocks, rank_sum = blocks + 1, rank_sum + Ws[k].shape[1]
        if arg < 0 or pb[k, 0] > best:
            best, arg = pb[k, 0], k
    return pb, np.array([np.sqrt(sq_all), dot_all, arg, best, blocks, rank_sum])
