"""cuadmm_lowrank_grad beside its yardsticks, behind a solve to 1e-3 with L = the factors of lowrank("X", 1e-6, rmax=16): the device time of
the chain (out8[6], HIP events) against one iteration of the same solver (the solve's wall time over its iterations), against the pieces a
caller would chain by hand in the same process -- block_multiply("dual", L), the whole of evaluate() (its SpMV is one launch of it; the
projections it also runs make this an upper bound of that share) and, last because it replaces the iterate, the pass of set_lowrank(X=L) --
and the whole Python call by wall clock.  One warm-up call, then REPS calls each; medians.
    python tools/probe_lowrank_grad.py [name ...]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuadmm_amd
from tests.conftest import load_npz_problem
from tests.helpers import problem_to_amd

REPS = 11
SIGMA = 1.0

for name in sys.argv[1:] or ["pendulum_N=80", "PushBox_N=30_MOMENT"]:
    a = problem_to_amd(load_npz_problem(name))
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(a)
    t = time.perf_counter()
    s.solve(100000, 1e-3, 500, 50, 100, 11000, 1.05)
    iter_ms = 1e3 * (time.perf_counter() - t) / s.info_iter_num
    f = s.lowrank("X", tol=1e-6, rmax=16)
    res = [s.lowrank_grad(f["L"], None, SIGMA) for _ in range(REPS + 1)]
    t = time.perf_counter()
    s.lowrank_grad(f["L"], None, SIGMA)
    call_ms = 1e3 * (time.perf_counter() - t)
    med = lambda v: float(np.median(v[1:]))
    lg_ms = med([r["ms"] for r in res])
    bm_ms = med([s.block_multiply("dual", f["L"])["ms"] for _ in range(REPS + 1)])
    ev_ms = med([s.evaluate()["ms"] for _ in range(REPS + 1)])
    lo_ms = med([s.set_lowrank(X=f["L"])["X"]["ms"] for _ in range(REPS + 1)])
    r0 = res[0]
    print("%-22s blocks %5d vec_len %9d con_num %7d rank sum %6d | iterations %5d, one %.3f ms | lowrank_grad %.4f ms (first %.4f), / iteration %.3f, whole call %.3f ms wall | "
          "block_multiply dual %.4f ms, evaluate %.4f ms, set_lowrank pass %.4f ms, their sum %.4f ms | sigma %g: f %.6e, <C, x> %.6e, y'r %.6e, ||r|| %.6e, ||G||_F %.6e, <L, G> %.6e"
          % (name, len(a.blk_vals), a.vec_len, a.con_num, int(sum(m.shape[1] for m in f["L"])), s.info_iter_num, iter_ms, lg_ms, r0["ms"], lg_ms / iter_ms, call_ms, bm_ms, ev_ms,
             lo_ms, bm_ms + ev_ms + lo_ms, SIGMA, r0["f"], r0["cx"], r0["yr"], r0["rnorm"], r0["gnorm"], r0["lg"]), flush=True)
