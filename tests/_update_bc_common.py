"""Shared by tests/test_gpu_update_bc.py and its two-process worker: the deterministic perturbation of b / C and small helpers."""
import numpy as np

INFO = ("errRp", "errRd", "pobj", "dobj", "relgap", "sig", "bscale", "Cscale")


def perturb(idx, val, n):
    """(idx, val) of a sparse vector of length n -> every nonzero scaled by 1 + 0.05 cos(i) (i: its index), the middle nonzero
    dropped, and the smallest index without an entry added with 0.05 times the mean magnitude."""
    idx, val = np.asarray(idx, np.int64), np.asarray(val, np.float64)
    assert idx.size >= 1 and idx.size < n, "the base vector needs an entry to drop and a free index to add"
    v = val * (1.0 + 0.05 * np.cos(idx.astype(np.float64)))
    keep = np.ones(idx.size, bool)
    keep[idx.size // 2] = False
    free = np.setdiff1d(np.arange(min(n, idx.size + 1)), idx)[0]
    new_idx = np.concatenate([idx[keep], [free]])
    new_val = np.concatenate([v[keep], [0.05 * float(np.mean(np.abs(val)))]])
    return new_idx.astype(np.int32), new_val


def thin(idx, val, every=7):
    """drops every `every`-th entry: a dense synthetic b / C becomes a sparse one (so that perturb() has an index to add)"""
    keep = np.arange(np.asarray(idx).size) % every != every - 1
    return np.asarray(idx, np.int32)[keep], np.asarray(val, np.float64)[keep]


def init_with(s, a, b, C, X0=None, y0=None, S0=None, sig=1.0):
    """cuadmm_init of solver s with A / blk of problem a and the sparse pairs b = (idx, val), C = (idx, val)"""
    return s.init(15, 30, a.vec_len, a.con_num, a.At_csc_col_ptrs, a.At_csc_row_ids, a.At_csc_vals, a.At_nnz, b[0], b[1], len(b[0]),
                  C[0], C[1], len(C[0]), a.blk_vals, a.mat_num, X0, y0, S0, sig)


def snapshot(s):
    st = s.state()
    return [s.info_arr(k).copy() for k in INFO] + [np.array([st[k] for k in sorted(st)]), np.array([s.info_iter_num]), s.X, s.y, s.S]
