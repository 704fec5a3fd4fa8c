"""The recurrence of cuadmm_lowrank_refine in numpy doubles (csrc/lowrank_refine.h, include/cuadmm_amd.h): every operation below is one
IEEE operation on float64 arrays, so the results are the bits the kernels and cuadmm_cg_update must return.  Shared by
tests/test_lowrank_refine_host.py and tests/test_gpu_lowrank_refine.py."""
import numpy as np

from tests._block_mult_twin import LD, U

TRACE = ("gg", "go", "gd", "beta", "slope", "restart", "c0", "c1", "c2", "c3", "c4", "t", "f", "ms")
SLOTS, THREADS = 256, 256                      # kBrSlots, kBrThreads (csrc/block_reduce.h)
COUNTS = (1, 2, 3, 255, 256, 257, 511, 513, SLOTS * THREADS + 1)      # the last: one more than a full stride of the slot-partial kernel


def grad(W, unit):
    """G = 2.0 * (W * unit): two roundings (the doubling is exact)"""
    return 2.0 * (np.asarray(W, np.float64) * np.float64(unit))


def cg_update(gg, go, gd, gg_prev, first):
    """(beta, slope, restart) by the formula of the header, in float64"""
    gg, go, gd, gg_prev = (np.float64(v) for v in (gg, go, gd, gg_prev))
    beta = np.float64(0.0)
    if not first and gg_prev != 0.0:
        with np.errstate(all="ignore"):
            pr = (gg - go) / gg_prev
        beta = pr if pr > 0.0 else np.float64(0.0)
    with np.errstate(all="ignore"):
        slope = -gg + beta * gd
    restart = bool(first) or not slope < 0.0
    return (0.0 if restart else float(beta)), float(slope), restart


def direction(G, D_old, beta, restart, root):
    """(D, Ds): D = -G + beta D_old, or -G on a restart; Ds = D root"""
    G = np.asarray(G, np.float64)
    D = -G if restart else -G + np.float64(beta) * np.asarray(D_old, np.float64)
    return D, D * np.float64(root)


def step(L, D, t, root):
    """(L + t D, (L + t D) root)"""
    Ln = np.asarray(L, np.float64) + np.float64(t) * np.asarray(D, np.float64)
    return Ln, Ln * np.float64(root)


def dots_ref(G, G_old, D_old):
    """[(sum, sum of absolute values)] of G G, G G_old, G D_old in longdouble over the float64 vectors"""
    g = np.asarray(G).astype(LD)
    return [(np.sum(g * np.asarray(v).astype(LD)), np.sum(np.abs(g * np.asarray(v).astype(LD)))) for v in (G, G_old, D_old)]


def dots_bound(count, bar):
    """The slot-sum bound the project uses for lrl_sums (tests/test_gpu_lowrank_line.py: test_quartic_sums): a thread adds at most
    count / 65536 terms, the workgroup's tree and the 256 slots follow, and the product of a term is rounded once -- all inside
    (count / 256 + 264) u sum |terms|."""
    return (count / 256 + 264) * LD(U) * LD(bar)


def view(a, shift, guard=None):
    """a copy of `a` (with `guard` appended where given) that starts 8 * shift bytes behind a 16-byte boundary"""
    a = np.asarray(a, np.float64)
    n = a.size + (guard is not None)
    base = np.zeros(n + 3)
    at = (((base.ctypes.data >> 3) & 1) + shift) % 2
    v = base[at:at + n]
    v[:a.size] = a
    if guard is not None:
        v[-1] = guard
    assert ((v.ctypes.data >> 3) & 1) == shift
    return v
