"""cuadmm_lowrank_line beside its yardsticks, behind a solve to 1e-3 with L = the factors of lowrank("X", 1e-6, rmax=16) and D = -G of
lowrank_grad at L: the device time of the chain (out8[6], HIP events) against one lowrank_grad chain, against one iteration of the same
solver (the solve's wall time over its iterations), and the whole Python call by wall clock.  One warm-up call, then REPS calls each;
medians.  With --once: a solve and three calls only, for a kernel trace of the chain (the split between the outer-product pass, the
three SpMVs and the sums).
    python tools/probe_lowrank_line.py [--once] [name ...]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuadmm_amd
from tests.conftest import load_npz_problem
from tests.helpers import problem_to_amd

args = [a for a in sys.argv[1:] if a != "--once"]
REPS = 2 if "--once" in sys.argv[1:] else 11
SIGMA = 1.0

for name in args or ["pendulum_N=80", "PushBox_N=30_MOMENT"]:
    a = problem_to_amd(load_npz_problem(name))
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(a)
    t = time.perf_counter()
    s.solve(100000, 1e-3, 500, 50, 100, 11000, 1.05)
    iter_ms = 1e3 * (time.perf_counter() - t) / s.info_iter_num
    f = s.lowrank("X", tol=1e-6, rmax=16)
    g = [s.lowrank_grad(f["L"], None, SIGMA) for _ in range(REPS + 1)]
    D = [-G for G in g[0]["G"]]
    res = [s.lowrank_line(f["L"], D, None, SIGMA) for _ in range(REPS + 1)]
    t = time.perf_counter()
    s.lowrank_line(f["L"], D, None, SIGMA)
    call_ms = 1e3 * (time.perf_counter() - t)
    med = lambda v: float(np.median(v[1:]))
    ll_ms, lg_ms = med([r["ms"] for r in res]), med([r["ms"] for r in g])
    r0 = res[0]
    after = s.lowrank_grad([L + r0["t"] * d for L, d in zip(f["L"], D)], None, SIGMA)["f"]
    print("%-22s blocks %5d vec_len %9d con_num %7d rank sum %6d | iterations %5d, one %.3f ms | lowrank_line %.4f ms (first %.4f), lowrank_grad %.4f ms, "
          "line / grad %.2f, line / iteration %.3f, whole call %.3f ms wall | sigma %g: c = [%.6e, %.6e, %.6e, %.6e, %.6e], t* %.6e, f(t*) %.9e, "
          "lowrank_grad there %.9e, critical points %d"
          % (name, len(a.blk_vals), a.vec_len, a.con_num, int(sum(m.shape[1] for m in f["L"])), s.info_iter_num, iter_ms, ll_ms, r0["ms"], lg_ms, ll_ms / lg_ms,
             ll_ms / iter_ms, call_ms, SIGMA, *r0["coef"], r0["t"], r0["f"], after, r0["critical"]), flush=True)
