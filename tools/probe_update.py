"""cuadmm_update_bC against a second cuadmm_init: init seconds, update milliseconds (wall, with its final stream synchronisation),
iterations / seconds to 1e-3 from a cold init with the new data and from the update's warm start, and the svec pass's bandwidth
beside post_kernel's.  New data: every nonzero of b and C scaled by 1 + 0.05 cos(i).    python tools/probe_update.py [name ...]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuadmm_amd
from cuadmm_amd.synthetic import config_c2
from tests.conftest import load_npz_problem
from tests.helpers import problem_to_amd

CAP, TOL, PAR = 20000, 1e-3, (0, 50, 100, 5000, 1.05)           # the command line's solve parameters


def load(name):
    if name == "C2":
        q = config_c2()
        return cuadmm_amd.Problem(q.vec_len, q.con_num, q.blk, q.At_col_ptrs, q.At_row_ids, q.At_vals, q.b_idx, q.b_vals, q.C_idx, q.C_vals)
    return problem_to_amd(load_npz_problem({"c1": "PlanarHand_N=1_MOMENT", "c5": "pendulum_N=80"}.get(name, name)))


def init(a, b, C, **kw):
    s = cuadmm_amd.SDPSolver(verbose=False, **kw)
    t = time.perf_counter()
    s.init(15, 30, a.vec_len, a.con_num, a.At_csc_col_ptrs, a.At_csc_row_ids, a.At_csc_vals, a.At_nnz, b[0], b[1], len(b[0]), C[0], C[1], len(C[0]),
           a.blk_vals, a.mat_num, None, None, None, 1.0)
    return s, time.perf_counter() - t


def to_tol(s):
    t = time.perf_counter()
    s.solve(CAP, TOL, *PAR)
    return s.info_iter_num, time.perf_counter() - t


for name in sys.argv[1:] or ["C2", "c1", "c5", "PushT_N=30_MOMENT", "PushBox_N=30_MOMENT"]:
    a = load(name)
    b, C = (a.b_indices, a.b_vals), (a.C_indices, a.C_vals)
    b2 = (b[0], b[1] * (1 + 0.05 * np.cos(b[0].astype(float))))
    C2 = (C[0], C[1] * (1 + 0.05 * np.cos(C[0].astype(float))))
    s, init_s = init(a, b, C, profile=1)
    it0, s0 = to_tol(s)
    s.reset_profile()
    t = time.perf_counter()
    s.update_bC(b2[0], b2[1], C2[0], C2[1], True, 0.0)
    update_ms = 1e3 * (time.perf_counter() - t)
    pr = s.profile()["post_proj"]                                 # the svec pass is the update's only entry in this class
    tbs = pr["bytes_per_launch"] / pr["ms"] * 1e-9 if pr["ms"] > 0 else float("nan")
    it_w, s_w = to_tol(s)
    del s
    c, init2_s = init(a, b2, C2)
    it_c, s_c = to_tol(c)
    del c
    print("%-20s L %9d m %7d | init_s %6.2f (again with the new data %6.2f) update_ms %7.2f | first solve %5d it %6.2f s | new data to 1e-3: cold %5d it %6.2f s, "
          "warm %5d it %6.2f s | svec pass %.3f ms, %.2f TB/s" % (name, a.vec_len, a.con_num, init_s, init2_s, update_ms, it0, s0, it_c, s_c, it_w, s_w, pr["ms"], tbs), flush=True)
    if name == "C2":                                              # post_kernel on the same box: the unfused iteration's post step, 48 L bytes
        u, _ = init(a, b, C, profile=1, options={"fuse": 0})
        u.solve(60, 0.0, 0, 50, 100, 0, 1.05)
        pp = u.profile()["post_proj"]
        print("%-20s post_kernel (unfused, mode 0): %.3f ms per launch, %.2f TB/s" % (name, pp["ms"] / pp["launches"], pp["bytes_per_launch"] * pp["launches"] / pp["ms"] * 1e-9), flush=True)
        del u
