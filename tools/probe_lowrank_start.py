"""cuadmm_set_lowrank beside its yardsticks, behind a solve to 1e-3 with the factors of lowrank("X", 1e-6, rmax=16): the kernel pass
(out4[2], HIP events) against one iteration of the same solver (the solve's wall time over its iterations), against the route without it
(L L' and svec per block in numpy, then set_XyS; wall clock) and against a hipMemsetAsync of the same 8 vec_len bytes timed with events in
the same process.  One warm-up call, then REPS calls each; medians.    python tools/probe_lowrank_start.py [name ...]"""
import ctypes as C
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuadmm_amd
from cuadmm_amd.devbuf import Dev
from tests.conftest import load_npz_problem
from tests.helpers import problem_to_amd

REPS = 11
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))


def memset_ms(nbytes):
    d = Dev(shape=(nbytes // 8,))
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    out = []
    for _ in range(REPS + 1):
        ms = C.c_float(0)
        assert hip.hipEventRecord(e0, None) == 0 and hip.hipMemsetAsync(d.ptr, 0, C.c_size_t(nbytes), None) == 0 and hip.hipEventRecord(e1, None) == 0
        assert hip.hipEventSynchronize(e1) == 0 and hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        out.append(ms.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return float(np.median(out[1:]))


def host_route(s, blk, Ls):
    """what a caller does without set_lowrank: every L_k L_k' and its svec on the host, the whole vector through set_XyS"""
    t = time.perf_counter()
    X = s.X                                                                   # (the unconstrained blocks keep their values)
    at = 0
    for n, Lk in zip(blk, Ls):
        if n < 0:
            at += -n
            continue
        M = Lk @ Lk.T
        ii, jj = np.tril_indices(n)
        X[at:at + ii.size] = np.where(ii == jj, M[ii, jj], M[ii, jj] * 1.4142135623730951)
        at += ii.size
    s.set_XyS(X=X)
    return 1e3 * (time.perf_counter() - t)


for name in sys.argv[1:] or ["pendulum_N=80", "PushBox_N=30_MOMENT"]:
    a = problem_to_amd(load_npz_problem(name))
    blk = [int(n) for n in a.blk_vals]
    s = cuadmm_amd.SDPSolver(verbose=False)
    s.init_problem(a)
    t = time.perf_counter()
    s.solve(100000, 1e-3, 500, 50, 100, 11000, 1.05)
    iter_ms = 1e3 * (time.perf_counter() - t) / s.info_iter_num
    f = s.lowrank("X", tol=1e-6, rmax=16)
    res = [s.set_lowrank(X=f["L"])["X"] for _ in range(REPS + 1)]
    t = time.perf_counter()
    s.set_lowrank(X=f["L"])
    call_ms = 1e3 * (time.perf_counter() - t)
    kern = float(np.median([r["ms"] for r in res[1:]]))
    host = float(np.median([host_route(s, blk, f["L"]) for _ in range(4)][1:]))
    ms0 = memset_ms(8 * a.vec_len)
    print("%-22s blocks %5d vec_len %9d rank sum %6d staged %9.0f B | iterations %5d, one %.3f ms | set_lowrank kernel %.4f ms (first %.4f), whole call %.3f ms wall | "
          "numpy + set_XyS %.2f ms wall | hipMemsetAsync of %d B %.4f ms | kernel / memset %.2f, kernel / iteration %.3f, host route / call %.0f"
          % (name, len(blk), a.vec_len, res[0]["rank_sum"], res[0]["bytes_staged"], s.info_iter_num, iter_ms, kern, res[0]["ms"], call_ms, host, 8 * a.vec_len, ms0,
             kern / ms0, kern / iter_ms, host / call_ms), flush=True)
