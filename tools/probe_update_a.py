"""cuadmm_update_A against a second cuadmm_init: init seconds (first, and again with the new values), update milliseconds (wall) with the
split of cuadmm_get_update_info (host numeric factor, device part of the y-solve rebuild, bytes uploaded), and the value pass's bandwidth
(cuadmm_get_update_pass_info: the kernel alone between two events; per CSR slot 4 bytes of map, 8 gathered, 8 stored) beside
update_svec_kernel's on the same box (32 bytes per svec element).
New values: every nonzero of A scaled by 1 + 0.05 cos(i).    python tools/probe_update_a.py [name ...]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuadmm_amd
from cuadmm_amd.synthetic import config_c2
from tests.conftest import load_npz_problem
from tests.helpers import problem_to_amd


def load(name):
    if name == "C2":
        q = config_c2()
        return cuadmm_amd.Problem(q.vec_len, q.con_num, q.blk, q.At_col_ptrs, q.At_row_ids, q.At_vals, q.b_idx, q.b_vals, q.C_idx, q.C_vals)
    return problem_to_amd(load_npz_problem({"c1": "PlanarHand_N=1_MOMENT", "c5": "pendulum_N=80"}.get(name, name)))


def init(a, vals, **kw):
    s = cuadmm_amd.SDPSolver(verbose=False, **kw)
    t = time.perf_counter()
    s.init(15, 30, a.vec_len, a.con_num, a.At_csc_col_ptrs, a.At_csc_row_ids, vals, a.At_nnz, a.b_indices, a.b_vals, len(a.b_indices),
           a.C_indices, a.C_vals, len(a.C_indices), a.blk_vals, a.mat_num, None, None, None, 1.0)
    return s, time.perf_counter() - t


for name in sys.argv[1:] or ["C2", "c1", "c5", "PushBox_N=30_MOMENT", "PushT_N=30_MOMENT"]:
    a = load(name)
    v = np.asarray(a.At_csc_vals, np.float64)
    v2 = v * (1 + 0.05 * np.cos(np.arange(v.size, dtype=float)))
    s, init_s = init(a, v, profile=1)
    s.solve(20, 0.0, 0, 50, 100, 5000, 1.05)
    s.update_A(v2, True)                                          # the first update builds the index maps
    first_ms = s.update_info()[1]
    s.solve(20, 0.0, 0, 50, 100, 5000, 1.05)
    t = time.perf_counter()
    s.update_A(v, True)
    wall_ms = 1e3 * (time.perf_counter() - t)
    u = s.update_info()
    ps = s.update_pass_info()                                     # each pass timed alone by its own events
    gbs = lambda ms, nbytes: nbytes / ms * 1e-6 if ms > 0 else float("nan")
    del s
    c, init2_s = init(a, v2)
    del c
    print("%-20s L %9d m %7d nnz %9d | init_s %6.2f (again with the new values %6.2f) | update_A ms: first %8.2f, then %8.2f (host factor %8.2f, "
          "device y-solve %8.2f, %.1f MB up, orderings %d) | value pass %.3f ms %.0f GB/s, svec pass %.3f ms %.0f GB/s"
          % (name, a.vec_len, a.con_num, a.At_nnz, init_s, init2_s, first_ms, wall_ms, u[2], u[3], u[5] * 1e-6, int(u[4]), ps[0], gbs(ps[0], ps[1]), ps[2], gbs(ps[2], ps[3])), flush=True)
