"""Writes tests/golden/accel_twin_traj.json: the trajectories of the numpy twin of the accelerated iteration (tests/_accel_twin.py)
that tests/test_gpu_accel.py compares the engine with, and the sensitivity behind their tolerance.

    python -m tests.golden.make_accel_traj

Per input and phase (ADMM: switch_admm = 0, sGS: 11000; hinf12 and closed also with the switch at iteration 10), accel = 5, 60 iterations: the info arrays, the accept / reject decisions,
the counts, and `spread`: the largest relative difference of the info arrays between that run and one whose every gamma_j was
multiplied by 1 + 1e-13 cos(j) (ATOL floors of tests/test_gpu_moment_parity.py).  tests/test_accel_host.py re-derives the small
entries from the twin, so the file cannot drift from it unnoticed.
"""
import json
import os
import tempfile

import numpy as np

from oracle import cuadmm_oracle as orc
from tests._accel_twin import accel_solve

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("errRp", "errRd", "pobj", "dobj", "relgap", "sig")
ITERS, MEM = 60, 5
INPUTS = ("hinf12", "ublock", "closed", "pendulum_N=80")
CROSS, CROSS_INPUTS = 10, ("hinf12", "closed")     # sGS until iteration 10, then ADMM with the best-iterate bookkeeping


def oracle_problem(name):
    from tests.test_gpu_accel import amd_problem
    from tests.test_gpu_moment_parity import load_problem
    if name in ("ublock", "closed", "mixed"):
        a = amd_problem(name)
        return orc.Problem(a.vec_len, a.con_num, a.blk_vals, a.At_csc_col_ptrs, a.At_csc_row_ids, a.At_csc_vals, a.b_indices, a.b_vals,
                           a.C_indices, a.C_vals)
    return load_problem(name, tempfile.mkdtemp())


def run(p, sw, perturb=0.0, iters=ITERS, mem=MEM):
    o = orc.OracleSolver().init_problem(p)
    info, log = accel_solve(o, iters, 0.0, 0, 50, 100, sw, 1.05, accel=mem, gamma_perturb=perturb)
    return {nm: list(map(float, getattr(info, nm))) for nm in NAMES}, log


def entry(p, sw):
    from tests.test_gpu_moment_parity import ATOL
    a, log = run(p, sw)
    b, _ = run(p, sw, 1e-13)
    spread = 0.0
    for nm in NAMES[:-1]:
        x, y = np.array(a[nm]), np.array(b[nm])
        spread = max(spread, float(np.max(np.maximum(np.abs(x - y) - ATOL[nm], 0.0) / np.maximum(np.abs(x), 1e-300))))
    return dict(a, decisions=[[int(i), d] for i, d in log.decisions], first_accept=log.first_accept, taken=log.taken, accepted=log.accepted,
                rejected=log.rejected, restarts=log.restarts, spread=spread)


def main():
    out = {}
    for name in INPUTS:
        p = oracle_problem(name)
        for sw in (0, 11000) + ((CROSS,) if name in CROSS_INPUTS else ()):
            e = entry(p, sw)
            out["%s/%d" % (name, sw)] = e
            print(name, sw, "taken", e["taken"], "accepted", e["accepted"], "rejected", e["rejected"], "restarts", e["restarts"],
                  "first accept", e["first_accept"], "spread %.3e" % e["spread"], flush=True)
    with open(os.path.join(HERE, "accel_twin_traj.json"), "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
