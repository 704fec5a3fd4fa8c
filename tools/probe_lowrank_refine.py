"""cuadmm_lowrank_refine beside its yardsticks, behind a solve to 1e-3 with L = the factors of lowrank("X", 1e-6, rmax=16), sigma = 1,
10 steps: the device interval per step (the trace's milliseconds, HIP events) against one lowrank_grad chain plus one lowrank_line
chain of the same process, and the wall time per step of the whole call against lowrank_descent (one lowrank_grad and one lowrank_line
Python call per step) on the same input.  One warm-up, then REPS runs each; medians.
    python tools/probe_lowrank_refine.py [name ...]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuadmm_amd
from tests.conftest import load_npz_problem
from tests.helpers import problem_to_amd

REPS, STEPS, SIGMA = 11, 10, 1.0


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t), out


for name in sys.argv[1:] or ["pendulum_N=80", "PushBox_N=30_MOMENT"]:
    a = problem_to_amd(load_npz_problem(name))
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(a)
    s.solve(100000, 1e-3, 500, 50, 100, 11000, 1.05)
    f = s.lowrank("X", tol=1e-6, rmax=16)
    g = [s.lowrank_grad(f["L"], None, SIGMA) for _ in range(REPS + 1)]
    D = [-G for G in g[0]["G"]]
    ln = [s.lowrank_line(f["L"], D, None, SIGMA) for _ in range(REPS + 1)]
    rf = [wall(lambda: s.lowrank_refine(f["L"], None, SIGMA, STEPS)) for _ in range(REPS + 1)]
    de = [wall(lambda: s.lowrank_descent(f["L"], None, SIGMA, STEPS)) for _ in range(REPS + 1)]
    med = lambda v: float(np.median(v[1:]))
    r0, d0 = rf[0][1], de[0][1]
    n = max(len(r0["trace"]), 1)
    step_ms = med([np.mean([t["ms"] for t in r[1]["trace"]]) for r in rf])
    loop_ms = med([r[1]["ms"] for r in rf])
    lg_ms, ll_ms = med([r["ms"] for r in g]), med([r["ms"] for r in ln])
    print("%-22s blocks %5d rank sum %6d factor doubles %8d | refine: %d steps, reason %d, f %.9e -> %.9e | device per step %.4f ms (loop %.4f ms / %d), "
          "lowrank_grad chain %.4f + lowrank_line chain %.4f = %.4f ms | wall per step: refine %.3f ms (whole call %.3f ms), lowrank_descent %.3f ms "
          "(whole call %.3f ms, %d steps, last f %.9e), ratio %.1f"
          % (name, len(a.blk_vals), int(sum(m.shape[1] for m in f["L"])), int(sum(m.size for m in f["L"])), r0["steps"], r0["reason"], r0["f0"], r0["f"], step_ms,
             loop_ms, n, lg_ms, ll_ms, lg_ms + ll_ms, med([r[0] for r in rf]) / n, med([r[0] for r in rf]), med([r[0] for r in de]) / max(len(d0["trace"]), 1),
             med([r[0] for r in de]), len(d0["trace"]), d0["trace"][-1]["predicted"], (med([r[0] for r in de]) / max(len(d0["trace"]), 1)) / (med([r[0] for r in rf]) / n)),
          flush=True)
