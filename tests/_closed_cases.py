"""Deterministic block-diagonal problems whose rows of A are placed by hand, for the closed-block iteration (psd_sign_closed.h).

make_synthetic gives every block the same number of rows and draws every row's slots uniformly, so a block's record (ClosedRec,
psd_fuse.h) is only ever filled one way: one scatter round (two on a rare collision), off-diagonal slots, rows of equal length.
build(blk, structure, seed) places the rows so that the record's other shapes occur in every block, and the block lists below
hold classes made only of 16s, 32s, 48s or 64s, which is what selects the FULL instantiations of the kernels (PsdRange::full).

Everything but the placement follows make_synthetic: slot t of a block is (column ii[t], row jj[t]) of np.tril_indices(n) (slot 0
is (0,0), slot len - 1 is (n-1,n-1), the diagonal slot of index i is i (i + 3) / 2), the arrays are the CSC of A^T sorted by
constraint and svec row, X0 = G G^T / n + I, S0 = H H^T / n + I, b = A svec(X0), C = svec(S0) + A^T y0: strictly feasible.

Draw order (numpy PCG64(seed)): per size group (ascending n) G then H ~ N(0,1)^(cnt,n,n); then block by block, in the order of
the list: one permutation of the block's slots, then the block's values ~ N(0,1), row by row; finally y0 ~ N(0,1)^m.
The one departure from N(0,1): the value of a row with a SINGLE nonzero is redrawn until |v| >= MIN_SINGLE.  Its square is the
row's diagonal entry of A_k A_k^T; beside a row of 57 nonzeros (squared norm about 57) cond <= 1e4 needs |v| >= 0.076, which 6 %
of N(0,1) draws miss -- with some 1 000 such rows per case no seed would meet the bound the host test asserts.
"""
import numpy as np

from cuadmm_amd.synthetic import _offsets, _pack

STRUCTURES = ("dense", "stacked", "ragged", "rowless")
MAX_ROWS, MAX_NNZ = 8, 64                    # kClosedMaxRows, kFuseRowsMax (psd_fuse.h)
LONG_ROW = 57                                # ragged: 57 + 7 x 1 = 64 nonzeros
MIN_SINGLE = 0.25
RAGGED_LEN = (1, 2, 3, 5, 8, 13, 4)          # row lengths of a ragged block with fewer than 8 rows (row 0: one diagonal slot)

EDGES = [9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]


def diag_slot(i):
    return i * (i + 3) // 2


def is_rowless(k):
    """rowless: every fourth block has no rows"""
    return k % 4 == 3


def _dense_rows(n, perm):
    """8 rows x 8 nonzeros on 64 distinct slots, slot 0 and slot len - 1 among them (rows 0 and 7).  A block with fewer than 64
    slots (n <= 10) cannot keep them distinct: the walk wraps round its slots, so that no ROW repeats one (multiplicity <= 2)."""
    L = n * (n + 1) // 2
    inner = [int(s) for s in perm if s not in (0, L - 1)]
    seq = [0] + inner[:min(L, MAX_NNZ) - 2] + [L - 1]
    return [[seq[(8 * r + q) % len(seq)] for q in range(8)] for r in range(MAX_ROWS)]


def _stacked_rows(n, perm):
    """8 rows, each with slot 0 and slot len - 1 (multiplicity 8: eight scatter rounds); rows 0, 3 and 7 share one off-diagonal
    slot (multiplicity 3); every other nonzero on a slot of its own.  Rows of 8 nonzeros where the block has the 48 slots that
    needs (64 nonzeros), shorter rows below that."""
    L = n * (n + 1) // 2
    rl = min(8, (L + 16) // 8)
    diag = set(diag_slot(i) for i in range(n))
    inner = [int(s) for s in perm if s not in (0, L - 1)]
    shared = next(s for s in inner if s not in diag)
    rest = iter(s for s in inner if s != shared)
    rows = []
    for r in range(MAX_ROWS):
        own = rl - (3 if r in (0, 3, 7) else 2)
        rows.append([0, L - 1] + ([shared] if r in (0, 3, 7) else []) + [next(rest) for _ in range(own)])
    return rows


def _ragged_rows(n, perm, k):
    """Block k has 1 + k % 8 rows.  Fewer than 8: lengths RAGGED_LEN on distinct slots, row 0 a single nonzero on a diagonal
    slot (first, last, middle in turn).  8 rows: one row of 57 nonzeros (capped at the block's slots less one), at a position
    that moves with k, holding slot 0 and slot len - 1, beside seven single-nonzero rows that sit on slots of the long row
    (multiplicity 2, and a dense column in the block's factor of A A^T), the first of them on a diagonal slot."""
    L = n * (n + 1) // 2
    nk = 1 + k % 8
    d0 = (0, L - 1, diag_slot(n // 2))[(k // 8) % 3]
    if nk < MAX_ROWS:
        rest = iter(int(s) for s in perm if s != d0)
        return [[d0]] + [[next(rest) for _ in range(min(RAGGED_LEN[r], L - 1))] for r in range(1, nk)]
    ll = min(LONG_ROW, L - 1)
    inner = [int(s) for s in perm if s not in (0, L - 1)]
    long_row = [0, L - 1] + inner[:ll - 2]
    singles = [[d0]] + [[s] for s in [t for t in inner[:ll - 2] if t != d0][:6]]
    pos = (k // 8) % MAX_ROWS
    return singles[:pos] + [long_row] + singles[pos:]


def block_rows(n, structure, k, perm):
    """The slots of every row of block k (size n), perm = the block's permutation of its slots."""
    if structure == "dense":
        return _dense_rows(n, perm)
    if structure == "stacked":
        return _stacked_rows(n, perm)
    if structure == "ragged":
        return _ragged_rows(n, perm, k)
    if structure == "rowless":
        return [] if is_rowless(k) else _dense_rows(n, perm)
    raise ValueError("unknown structure %r" % (structure,))


def build(blk, structure, seed):
    """-> (vec_len, con_num, blk, At_col_ptrs, At_row_ids, At_vals, b_idx, b_vals, C_idx, C_vals): the arguments of
    cuadmm_amd.Problem and oracle.cuadmm_oracle.Problem.  Constraints are numbered round by round over the blocks (row r of
    every block that has one, blocks ascending), the interleaving make_synthetic uses."""
    rng = np.random.Generator(np.random.PCG64(seed))
    blk = np.asarray(blk, dtype=np.int64)
    off = _offsets(blk)
    nb, L = blk.size, int(off[-1])
    groups = [(int(n), np.nonzero(blk == n)[0]) for n in sorted(set(int(x) for x in blk))]
    X0m, S0m = [], []
    for n, ids in groups:
        G = rng.standard_normal((ids.size, n, n))
        H = rng.standard_normal((ids.size, n, n))
        X0m.append(G @ np.swapaxes(G, 1, 2) / n + np.eye(n)[None])
        S0m.append(H @ np.swapaxes(H, 1, 2) / n + np.eye(n)[None])
    x0 = _pack(blk, off, groups, X0m)
    s0 = _pack(blk, off, groups, S0m)
    per_block = []
    for k in range(nb):
        n = int(blk[k])
        rows = block_rows(n, structure, k, rng.permutation(n * (n + 1) // 2))
        vals = []
        for sl in rows:
            v = rng.standard_normal(len(sl))
            while len(sl) == 1 and abs(v[0]) < MIN_SINGLE:
                v = rng.standard_normal(1)
            vals.append(v)
        per_block.append((rows, vals))
    con_of = {}
    m = 0
    for r in range(MAX_ROWS):
        for k in range(nb):
            if len(per_block[k][0]) > r:
                con_of[(k, r)] = m
                m += 1
    rows_l, cols_l, vals_l = [], [], []
    for k in range(nb):
        for r, (sl, v) in enumerate(zip(*per_block[k])):
            rows_l.append(off[k] + np.asarray(sl, np.int64))
            cols_l.append(np.full(len(sl), con_of[(k, r)], np.int64))
            vals_l.append(v)
    rows, cols, vals = np.concatenate(rows_l), np.concatenate(cols_l), np.concatenate(vals_l)
    order = np.lexsort((rows, cols))
    rows, cols, vals = rows[order].astype(np.int32), cols[order].astype(np.int32), vals[order]
    cp = np.zeros(m + 1, np.int32)
    np.add.at(cp, cols + 1, 1)
    cp = np.cumsum(cp).astype(np.int32)
    y0 = rng.standard_normal(m)
    b = np.zeros(m)
    np.add.at(b, cols, vals * x0[rows])
    aty = np.zeros(L)
    np.add.at(aty, rows, vals * y0[cols])
    Cv = s0 + aty
    b_idx = np.nonzero(b)[0].astype(np.int32)
    C_idx = np.nonzero(Cv)[0].astype(np.int32)
    return L, m, blk.astype(np.int32), cp, rows, vals, b_idx, b[b_idx], C_idx, Cv[C_idx]


# name -> (block list, structure, seed).  At least 256 blocks with rows everywhere: the device-side forest solve the closed path
# needs starts at 256 trees.  The seeds are the first for which every block meets cond(A_k A_k^T) <= 1e4 (test_closed_cases_host).
CASES = {
    "dense-16": ([16] * 256, "dense", 1),
    "dense-32": ([32] * 256, "dense", 1),
    "dense-48": ([48] * 256, "dense", 1),
    "dense-64": ([64] * 256, "dense", 1),
    "dense-edges": (EDGES * 22, "dense", 1),
    "stacked-16": ([16] * 256, "stacked", 1),
    "stacked-32": ([32] * 256, "stacked", 1),
    "stacked-edges": (EDGES * 22, "stacked", 1),
    "ragged-16": ([16] * 256, "ragged", 1),
    "ragged-32": ([32] * 256, "ragged", 1),
    "ragged-edges": (EDGES * 22, "ragged", 1),
    "rowless-16": ([16] * 344, "rowless", 1),
    "rowless-32": ([32] * 344, "rowless", 1),
    "rowless-edges": (EDGES * 29, "rowless", 1),
}

_built = {}


def case(name):
    """build(*CASES[name]), built once per process and shared: callers must not write into the arrays."""
    if name not in _built:
        _built[name] = build(*CASES[name])
        for a in _built[name]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _built[name]
