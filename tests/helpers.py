"""Small helpers for the GPU parity tests: device buffers through the C ABI (no torch needed)."""
import ctypes as C

import numpy as np

import cuadmm_amd
from cuadmm_amd._lib import check


from cuadmm_amd.devbuf import Dev  # noqa: E402,F401  (the tests' device buffers are the package's)


def opt_pairs(opts):
    """{"psd_*": value} -> (keys, vals, n) as the option-taking hooks expect them"""
    keys = (C.c_char_p * max(len(opts), 1))(*[k.encode() for k in opts])
    vals = np.array(list(opts.values()) + [0.0], np.float64)
    return keys, vals, len(opts)


def psd_project_gpu(x, blk, eig_rank=0, opts=None, steps=False):
    """opts: None = the plan's options come from the environment (cuadmm_op_psd_project_ex); a dict (an empty one too) = the built-in
    defaults changed by it and nothing else (cuadmm_op_psd_project_opts).  steps: -> (proj, Newton-Schulz steps per block)"""
    lib = cuadmm_amd.load()
    blk = np.ascontiguousarray(blk, dtype=np.int32)
    din = Dev(np.ascontiguousarray(x, dtype=np.float64))
    dout = Dev(shape=(x.size,), dtype=np.float64)
    dst = Dev(np.zeros(max(int(blk.size), 1), np.int32)) if steps else None
    if opts is None:
        check(lib.cuadmm_op_psd_project_ex(din.ptr, dout.ptr, blk.ctypes.data_as(C.c_void_p), int(blk.size), int(eig_rank), dst.ptr if steps else None, None))
    else:
        keys, vals, n = opt_pairs(opts)
        check(lib.cuadmm_op_psd_project_opts(din.ptr, dout.ptr, blk.ctypes.data_as(C.c_void_p), int(blk.size), int(eig_rank), keys,
                                             vals.ctypes.data_as(C.c_void_p), n, dst.ptr if steps else None, None))
    return (dout.get(), dst.get()[:blk.size]) if steps else dout.get()


def batch_eig_gpu(mats):
    """mats: (count, n, n) symmetric -> (W (count,n) ascending, V (count,n,n) with V[i][:,k] eigenvector k, info)."""
    lib = cuadmm_amd.load()
    count, n, _ = mats.shape
    colmajor = np.ascontiguousarray(np.swapaxes(mats, 1, 2))      # element (r,c) at c*n+r
    dm = Dev(colmajor)
    dw = Dev(shape=(count, n), dtype=np.float64)
    di = Dev(np.zeros(count, np.int32))
    check(lib.cuadmm_op_batch_eig(dm.ptr, dw.ptr, di.ptr, n, count, None))
    V = np.swapaxes(dm.get(), 1, 2)
    return dw.get(), V, di.get()


def problem_to_amd(p):
    """oracle Problem -> cuadmm_amd.Problem"""
    return cuadmm_amd.Problem(p.vec_len, p.con_num, p.blk, p.At_col_ptrs, p.At_row_ids, p.At_vals,
                              p.b_idx, p.b_vals, p.C_idx, p.C_vals)


# ----------------------------------------------------------------------------------------------------------------------
# Inputs and references of the op-level y-solve tests (tests/test_gpu_lead_solve.py, tests/test_lead_generators.py).
#
# A graph on the m constraints is turned into A = [diag(d) | one column per edge (two entries) | one column per clique]:
# A A^T then has exactly that graph as its pattern and is diagonally dominant for small edge weights.  HUB rows -- tied to
# hundreds of other rows and, through one clique column, to each other -- are what the minimum-degree ordering keeps for
# last, so a forced tail of as many columns holds them, and the leading elimination forest is the graph without them.
# ----------------------------------------------------------------------------------------------------------------------
import scipy.sparse as sp  # noqa: E402


class _Graph:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.n = 0
        self.edges = []
        self.cliques = []

    def nodes(self, count):
        first = self.n
        self.n += count
        return np.arange(first, first + count)

    def tree(self, count, chain=False):
        """count nodes; chain: a path (a deep elimination tree), else node i hangs under a random earlier node"""
        ids = self.nodes(count)
        for i in range(1, count):
            self.edges.append((ids[i], ids[i - 1] if chain else ids[self.rng.integers(0, i)]))
        return ids

    def matrix(self, weight=0.3, clique_weight=0.02):
        rng, m, ne = self.rng, self.n, len(self.edges)
        e = np.asarray(self.edges, dtype=np.int64).reshape(ne, 2)
        rows = [np.arange(m), e[:, 0], e[:, 1]]
        cols = [np.arange(m), m + np.arange(ne), m + np.arange(ne)]
        vals = [rng.uniform(3.0, 5.0, m), rng.uniform(0.5, 1.0, ne) * rng.choice([-1.0, 1.0], ne), weight * rng.uniform(0.5, 1.0, ne)]
        col = m + ne
        for members in self.cliques:
            rows.append(np.asarray(members)); cols.append(np.full(len(members), col)); col += 1
            vals.append(clique_weight * rng.uniform(0.5, 1.0, len(members)))
        A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(m, col))
        A.sort_indices()
        return A


def _add_hubs(g, k, trees, per_tree, reach=16, hubs=None):
    """k hub rows in one clique; every tree of `trees` (arrays of rows) gets `per_tree` ties into a set of at most `reach` hubs of its
    own -- fewer than a hub has neighbours among the hubs alone, so no leading row ever outgrows a hub's degree"""
    hubs = g.nodes(k) if hubs is None else hubs
    for ids in trees:
        mine = g.rng.choice(hubs, size=min(reach, k), replace=False)
        n = min(len(ids) * len(mine), max(1, int(per_tree * len(ids))))
        pairs = g.rng.choice(len(ids) * len(mine), size=n, replace=False)
        for q in pairs:
            g.edges.append((ids[q // len(mine)], mine[q % len(mine)]))
    g.cliques.append(hubs)
    return hubs


def lead_case(name):
    """-> (A (scipy CSC, m x n), k = the tail size to force, marks: dict of named ORIGINAL row numbers)"""
    if name == "small":                 # a few hundred small trees
        g = _Graph(11)
        _add_hubs(g, 64, [g.tree(int(s)) for s in g.rng.integers(20, 301, 240)], 0.5)
        return g.matrix(), 64, {}
    if name == "mixed":                 # small trees, trees beyond the 16 KB of a shared workgroup, one beyond a workgroup's LDS
        g = _Graph(12)
        sizes = list(g.rng.integers(20, 301, 60)) + [700, 1500, 3000, 4000, 6000]
        _add_hubs(g, 64, [g.tree(int(s)) for s in sizes], 0.3)
        return g.matrix(), 64, {}
    if name == "micro":                 # thousands of one- and two-node trees beside a few larger ones
        g = _Graph(13)
        parts = [g.tree(1) for _ in range(5000)] + [g.tree(2) for _ in range(4500)] + [g.tree(int(s)) for s in (3, 40, 150, 300)]
        _add_hubs(g, 64, parts, 0.5)
        return g.matrix(), 64, {}
    if name == "deep":                  # chains: elimination trees far deeper than any cut of the tree tops
        g = _Graph(14)
        chains = [g.tree(int(s), chain=True) for s in (150, 200, 260, 320, 400, 180, 220, 500)]
        bushes = [g.tree(int(s)) for s in g.rng.integers(5, 60, 40)]
        hubs = g.nodes(64)
        for ids in chains:              # every row of a chain tied to the same four hubs: its two ends stay the rows of least degree
            for h in g.rng.choice(hubs, size=4, replace=False):
                g.edges.extend((j, h) for j in ids)
        _add_hubs(g, 64, bushes, 0.5, hubs=hubs)
        return g.matrix(), 64, {}
    if name.startswith("long"):         # long127 / long128 / long129 / long2000: an isolated leading row tied to exactly that many hubs
        rows = int(name[4:])
        k = 256 if rows <= 200 else 2048
        g = _Graph(15 + rows)
        parts = [g.tree(int(s)) for s in g.rng.integers(3, 40, 60)]
        marked, lonely = g.nodes(1)[0], g.nodes(1)[0]
        hubs = _add_hubs(g, k, parts, 2.0, reach=100)
        for h in g.rng.choice(hubs, size=rows, replace=False):
            g.edges.append((marked, h))
        return g.matrix(weight=0.1, clique_weight=0.4 / k), k, {"marked": int(marked), "lonely": int(lonely)}
    if name == "forest":                # block-diagonal A A^T for the one-thread-per-tree solve (no tail)
        g = _Graph(16)
        for s in g.rng.integers(1, 65, 400):
            g.tree(int(s))
        return g.matrix(), 0, {}
    raise KeyError(name)


class Factor:
    """cuadmm_aat_create_split (tail forced to k columns; k = 0: cuadmm_aat_create) with its arrays as numpy views"""

    def __init__(self, A, k):
        lib = cuadmm_amd.load()
        self.lib, self.m, self.k, self.n1 = lib, A.shape[0], k, A.shape[0] - k
        cp, ri, vx = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        self.h = C.c_void_p()
        if k > 0:
            check(lib.cuadmm_aat_create_split(self.m, A.shape[1], P(cp), P(ri), P(vx), 1e-15, -k, C.byref(self.h)))
        else:
            check(lib.cuadmm_aat_create(self.m, A.shape[1], P(cp), P(ri), P(vx), 1e-15, C.byref(self.h)))
        assert lib.cuadmm_aat_tail_k(self.h) == k
        self.perm = np.ctypeslib.as_array(lib.cuadmm_aat_perm(self.h), shape=(self.m,)).copy()
        a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib.cuadmm_aat_factor_arrays(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        self.Lp = np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_int64)), shape=(self.m + 1,))[:self.n1 + 1].copy()
        nnz = int(self.Lp[-1])
        self.Li = np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_int)), shape=(max(nnz, 1),))[:nnz].copy()
        self.Lx = np.ctypeslib.as_array(C.cast(c, C.POINTER(C.c_double)), shape=(max(nnz, 1),))[:nnz].copy()
        self.D = np.ctypeslib.as_array(C.cast(d, C.POINTER(C.c_double)), shape=(self.m,))[:self.n1].copy()
        self.S = None
        if k > 0:                       # the Schur complement the tail factors: symmetric, from its lower triangle
            rp, ci, vv = C.POINTER(C.c_int64)(), C.POINTER(C.c_int)(), C.POINTER(C.c_double)()
            check(lib.cuadmm_aat_tail_schur(self.h, C.byref(rp), C.byref(ci), C.byref(vv)))
            rp = np.ctypeslib.as_array(rp, shape=(k + 1,)).copy()
            low = sp.csr_matrix((np.ctypeslib.as_array(vv, shape=(rp[-1],)).copy(), np.ctypeslib.as_array(ci, shape=(rp[-1],)).copy(), rp), shape=(k, k)).toarray()
            self.S = low + np.tril(low, -1).T

    def close(self):
        if self.h:
            self.lib.cuadmm_aat_free(self.h)
            self.h = None

    def forest(self):
        """leading elimination forest: parent, tree id per column, nodes per tree, height of the forest, tail rows per leading column"""
        n1, Lp, Li = self.n1, self.Lp, self.Li
        parent = np.full(n1, -1, np.int64)
        tail_rows = np.zeros(n1, np.int64)
        height = np.ones(n1, np.int64)
        for j in range(n1):
            rows = Li[Lp[j]:Lp[j + 1]]
            lead = rows[rows < n1]
            tail_rows[j] = rows.size - lead.size
            if lead.size:
                parent[j] = lead.min()
                height[parent[j]] = max(height[parent[j]], height[j] + 1)
        root = np.arange(n1)
        for j in range(n1 - 1, -1, -1):
            if parent[j] >= 0:
                root[j] = root[parent[j]]
        roots, tree_of, sizes = np.unique(root, return_inverse=True, return_counts=True)
        nnz11 = np.bincount(tree_of, weights=(Lp[1:] - Lp[:-1]) - tail_rows, minlength=roots.size).astype(np.int64)
        return dict(parent=parent, tree_of=tree_of, sizes=sizes, nnz11=nnz11, height=height, tail_rows=tail_rows)

    def solve_ref(self, rhs, dtype):
        """L D L^T x = rhs with the leading columns by column substitution in `dtype`; the tail block S (what the device factors itself)
        by a float64 Cholesky factorisation, refined against S in `dtype` until it stands still (np.longdouble) or not at all (float64)."""
        n1, Lp, Li = self.n1, self.Lp, self.Li
        Lx, D = self.Lx.astype(dtype), self.D.astype(dtype)
        x = np.array(rhs, dtype=dtype)
        for j in range(n1):
            if Lp[j + 1] > Lp[j] and x[j] != 0:
                x[Li[Lp[j]:Lp[j + 1]]] -= Lx[Lp[j]:Lp[j + 1]] * x[j]
        if self.k > 0:
            import scipy.linalg as sla
            cf = sla.cho_factor(self.S)
            z = x[n1:].copy()
            x2 = sla.cho_solve(cf, z.astype(np.float64)).astype(dtype)
            if dtype is not np.float64:
                Sd = self.S.astype(dtype)
                for _ in range(6):
                    x2 = x2 + sla.cho_solve(cf, (z - Sd @ x2).astype(np.float64)).astype(dtype)
            x[n1:] = x2
        x[:n1] /= D
        for j in range(n1 - 1, -1, -1):
            if Lp[j + 1] > Lp[j]:
                x[j] -= Lx[Lp[j]:Lp[j + 1]] @ x[Li[Lp[j]:Lp[j + 1]]]
        return x


def lead_rhs(ax, asmc, b, isig, dtype=np.longdouble):
    return -asmc.astype(dtype) + (b.astype(dtype) - ax.astype(dtype)) * dtype(isig)


def lead_vectors(m, seed, nrhs=1):
    rng = np.random.default_rng(seed)
    return tuple(np.ascontiguousarray(rng.standard_normal((nrhs, m))) for _ in range(3))


LEAD_INFO = ("ntrees", "max_levels", "n_small", "n_big", "n_stream", "n_micro", "n_long", "tops", "nT", "hybrid", "ready")


def lead_solve_gpu(fac, ax, asmc, b, isig, stream_only=0, small_kb=0, tops_level=0, force_hybrid=0):
    """cuadmm_op_lead_solve -> (y (nrhs, m) in the factor's order, info dict)"""
    ax, asmc, b = (np.ascontiguousarray(np.atleast_2d(v), dtype=np.float64) for v in (ax, asmc, b))
    nrhs, m = ax.shape
    assert m == fac.m and asmc.shape == ax.shape and b.shape == ax.shape
    y = np.full((nrhs, m), np.nan)
    info = np.full(11, -1, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    check(fac.lib.cuadmm_op_lead_solve(fac.h, m, int(stream_only), int(small_kb), int(tops_level), int(force_hybrid), P(ax), P(asmc), P(b),
                                       float(isig), nrhs, P(y), P(info)))
    return y, dict(zip(LEAD_INFO, (int(v) for v in info)))


# ----------------------------------------------------------------------------------------------------------------------
# The PSD projection on a PERSISTENT plan in the state the engine keeps it in (tests/test_gpu_psd_plan_state.py): schedule
# hints carried from projection to projection, descriptors re-sorted while the plan is live, a non-blocking caller's stream.
# ----------------------------------------------------------------------------------------------------------------------
class PlanHandle:
    """cuadmm_psd_plan_* with its buffers.  Plan options come from the environment at creation (PsdOptions::from_env)."""

    def __init__(self, blk):
        self.lib = cuadmm_amd.load()
        self.blk = np.ascontiguousarray(blk, dtype=np.int32)
        self.nblk = int(self.blk.size)
        n = self.blk.astype(np.int64)
        self.L = int(np.sum(n * (n + 1) // 2))
        self.h = C.c_void_p()
        check(self.lib.cuadmm_psd_plan_create(self.blk.ctypes.data_as(C.c_void_p), self.nblk, 0, C.byref(self.h)))
        self.din, self.dout, self.dsnap = (Dev(shape=(self.L,), dtype=np.float64) for _ in range(3))
        self.dsteps = Dev(np.zeros(self.nblk, np.int32))
        self.dhint = None
        self._nan = np.full(self.L, np.nan)
        self._zero = np.zeros(self.nblk, np.int32)
        self.hints_on = False
        self.hinted_projections = 0          # the plan ages its hints on every 16th of them

    def _up(self, dev, arr):
        arr = np.ascontiguousarray(arr, dtype=dev.dtype)
        assert arr.shape == dev.shape
        check(self.lib.cuadmm_memcpy_h2d(dev.ptr, arr.ctypes.data_as(C.c_void_p), dev.nbytes))

    def set_hint(self, hints, hint_max_n=512):
        """hints: mat_num ints uploaded into the plan's hint array, or None = hints off"""
        if hints is None:
            check(self.lib.cuadmm_psd_plan_set_hint(self.h, None, int(hint_max_n)))
            self.hints_on = False
            return
        if self.dhint is None:
            self.dhint = Dev(np.zeros(self.nblk, np.int32))
        self._up(self.dhint, hints)
        check(self.lib.cuadmm_psd_plan_set_hint(self.h, self.dhint.ptr, int(hint_max_n)))
        self.hints_on = True

    def get_hint(self):
        return self.dhint.get()

    def reorder(self, steps, async_=0, own_stream=0):
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        assert steps.size == self.nblk
        check(self.lib.cuadmm_psd_plan_reorder(self.h, steps.ctypes.data_as(C.c_void_p), int(async_), int(own_stream)))

    def project(self, x, own_stream=0):
        """-> (snap, Xproj, steps, fails): Xproj and the snapshot are prefilled with NaN and the steps with 0; `snap` is the copy of
        Xproj queued on the projection's stream right behind it, Xproj itself is read after a device-wide synchronisation."""
        self._up(self.din, x)
        self._up(self.dout, self._nan)
        self._up(self.dsnap, self._nan)
        self._up(self.dsteps, self._zero)
        fails = C.c_int(-1)
        check(self.lib.cuadmm_psd_plan_project_ordered(self.h, self.din.ptr, self.dout.ptr, self.dsnap.ptr, self.dsteps.ptr, int(own_stream),
                                                       C.byref(fails)))
        self.hinted_projections += self.dhint is not None and self.hints_on
        return self.dsnap.get(), self.dout.get(), self.dsteps.get(), fails.value

    def project_back_to_back(self, xs, own_stream=0):
        """The inputs one after the other into ONE output vector, as the engine does, with no upload or download between two projections (every buffer
        is uploaded before the first); each call still waits for its own stream, and for that stream only: -> the snapshots, one per input, and the last fail count."""
        dins = [Dev(np.ascontiguousarray(x, dtype=np.float64)) for x in xs]
        snaps = [Dev(self._nan) for _ in xs]
        self._up(self.dout, self._nan)
        self._up(self.dsteps, self._zero)
        fails = C.c_int(-1)
        for din, snap in zip(dins, snaps):
            check(self.lib.cuadmm_psd_plan_project_ordered(self.h, din.ptr, self.dout.ptr, snap.ptr, self.dsteps.ptr, int(own_stream),
                                                           C.byref(fails)))
            self.hinted_projections += self.dhint is not None and self.hints_on
        return [s.get() for s in snaps], fails.value

    def close(self):
        if self.h:
            check(self.lib.cuadmm_dev_sync())
            self.lib.cuadmm_psd_plan_destroy(self.h)
            self.h = None


# The inputs of tests/test_gpu_psd_plan_state.py and of its CPU precondition (tests/test_sign_schedule.py): block lists, spectrum families
# classes 0-4 and no sign path: the class of the largest blocks stays on the caller's stream, the others fork to a stream each
NO_SIGN = [3] * 8 + [8] * 8 + [9, 12, 15, 16] * 3 + [17, 24, 31, 32] * 3 + [33, 40, 48] * 2 + [49, 56, 63, 64] * 2
NO_SIGN = [int(n) for n in np.array(NO_SIGN)[np.random.default_rng(20240).permutation(len(NO_SIGN))]]
# ... beside a sign path (n >= 65: three padded sizes): the small classes share one side stream
WITH_SIGN = NO_SIGN + [65, 66, 91, 100, 120, 130, 200]
WITH_600 = WITH_SIGN + [600]

FAMILIES = ("randn", "lowrank", "graded", "psd", "nsd", "clustered", "moment")
STALE_FAMILIES = ("moment", "graded", "psd", "clustered", "randn", "zero")


def plan_matrix(n, kind, rng):
    """the spectrum families of tests/test_gpu_psd.py plus "moment" (rank 3 plus symmetric noise at 1e-12: ~30 lift steps) and "zero" """
    if kind == "zero":
        return np.zeros((n, n))
    if kind == "moment":
        U = rng.standard_normal((n, 3)); G = rng.standard_normal((n, n))
        return U @ U.T + 1e-12 * (G + G.T)
    from tests.test_gpu_psd import _spectrum_matrix          # (that module imports this one)
    return _spectrum_matrix(n, kind, rng)


# The launch variants of the batched-GEMM sign path (csrc/psd_large.hip) as tests/test_gpu_sign_variants.py forces them: name -> options (on top
# of the built-in defaults), block lists (the smallest shapes that reach the variant), spectrum families, and whether the group runs the
# multi-launch chain (ROLE 1 / 2 | 4 / 3) -- there the final product reads S or T by the parity of the step count, and both must occur.
# tests/test_sign_groups_host.py pins on the CPU that every (blk, opts) pair below reaches the variant it names.
_FOUR = ("randn", "lowrank", "graded", "clustered")
SIGN_VARIANTS = {
    "tile64_inline": dict(opts={"psd_lg_tile": 64}, blks=[[65], [129], [100, 100, 128]], kinds=FAMILIES, multi=True),
    "tile64_decide": dict(opts={"psd_lg_tile": 64, "psd_lg_decide": 2}, blks=[[65], [129, 192]], kinds=FAMILIES, multi=True),
    "tile32_inline": dict(opts={"psd_lg_cluster": 0}, blks=[[65], [270], [130, 192]], kinds=FAMILIES, multi=True),
    "tile32_decide": dict(opts={"psd_lg_cluster": 0, "psd_lg_decide": 2}, blks=[[65], [270]], kinds=FAMILIES, multi=True),
    "default_window": dict(opts={}, blks=[[720], [768]], kinds=_FOUR, multi=True),
    "inline_forced": dict(opts={"psd_lg_decide": 1}, blks=[[800]], kinds=("randn", "graded"), multi=True),
    "superblock32": dict(opts={"psd_lg_cluster": 0}, blks=[[512], [520]], kinds=_FOUR, multi=True),
    "superblock64": dict(opts={"psd_lg_tile": 64}, blks=[[1024], [1030]], kinds=("randn", "lowrank", "graded"), multi=True),
    "no_pad32": dict(opts={"psd_lg_pad32": 0}, blks=[[270], [410]], kinds=FAMILIES, multi=False),
}
SIGN_WS_CHUNKS = dict(opts={"psd_sign_ws_mb": 1}, blks=[[100] * 5, [150] * 3])
SIGN_NO_POLL = dict(opts={"psd_lg_cluster": 0, "psd_sign_sync": 0}, opts_poll={"psd_lg_cluster": 0, "psd_sign_sync": 1}, blk=[65, 100, 270])
SIGN_STEP_CAP = [({"psd_lg_cluster": 0}, [65, 100, 270]), ({}, [100, 128])]
SIGN_NON_FINITE = [({"psd_lg_cluster": 0}, [100, 65]), ({"psd_lg_tile": 64}, [100, 65]), ({}, [720])]
SIGN_ZERO_BLOCK = [({"psd_lg_tile": 64}, [100, 65]), ({"psd_lg_cluster": 0}, [100, 65]), ({"psd_lg_cluster": 0, "psd_lg_decide": 2}, [100, 65])]
SIGN_MIXED_CALL = dict(opts={}, blk=[65, 700, 130, 130, 40, 8, 700])


def block_scale(k):
    return 0.5 + 0.25 * k          # distinct per block: a block in another block's svec range cannot pass


_INPUTS = {}


def plan_input(blocks, tag):
    """-> (x, mats): tag = a family for every block, "mixed" = the seven families dealt round over the blocks (one zero block among them), or
    "sides" = moment blocks (~40 steps) on the side streams and zero blocks (one step) on the caller's: the join must wait"""
    key = (tuple(blocks), tag)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 + len(blocks) + sum(map(ord, tag)))
        main_min = 65 if max(blocks) > 64 else 33
        mats = []
        for k, n in enumerate(blocks):
            kind = tag
            if tag == "mixed":
                kind = "zero" if k == 5 else FAMILIES[k % len(FAMILIES)]
            elif tag == "sides":
                kind = "zero" if n >= main_min else "moment"
            mats.append(block_scale(k) * plan_matrix(n, kind, rng))
        x = np.concatenate([_orc().BlockIndex([M.shape[0]]).pack([M[None]]) for M in mats])
        _INPUTS[key] = (x, mats)
    return _INPUTS[key]


def _orc():
    from oracle import cuadmm_oracle
    return cuadmm_oracle


def plan_drift_input(blocks, k):
    """input k of 20 of a slowly drifting sequence x_0 + 0.02 k d with a jump to -x_0 at k = 10 (x_0: the mixed input)"""
    x0, _ = plan_input(blocks, "mixed")
    n = np.asarray(blocks, dtype=np.int64)
    d = np.random.default_rng(17).standard_normal(x0.size) * np.repeat([block_scale(q) for q in range(len(blocks))], n * (n + 1) // 2)
    return x0 + 0.02 * k * d if k < 10 else -x0 + 0.02 * (k - 10) * d
