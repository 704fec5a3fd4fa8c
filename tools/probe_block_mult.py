"""cuadmm_block_multiply beside its yardsticks, behind a solve to 1e-3 with V = the factors of lowrank("X", 1e-6, rmax=16): the device time of
block_multiply("S", V) and of block_multiply("dual", V) (out8[6], HIP events; the second with the formation of C - A'y) against one
iteration of the same solver (the solve's wall time over its iterations), against a device-to-device copy of the same 8 vec_len bytes timed
with events in the same process (the floor for reading the triangle once; the kernel reads every off-diagonal slot twice) and against the
route without the call (get_S, smat per block and the product in numpy; wall clock).  One warm-up call, then REPS calls each; medians.
    python tools/probe_block_mult.py [name ...]"""
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


def copy_ms(nbytes):
    a, b = Dev(shape=(nbytes // 8,)), Dev(shape=(nbytes // 8,))
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    out = []
    for _ in range(REPS + 1):
        ms = C.c_float(0)
        assert hip.hipEventRecord(e0, None) == 0 and hip.hipMemcpyAsync(b.ptr, a.ptr, C.c_size_t(nbytes), 3, None) == 0      # 3: device to device
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0 and hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        out.append(ms.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return float(np.median(out[1:]))


def host_route(s, blk, Vs):
    """what a caller does without block_multiply: the whole vector through get_S, smat per block and the product on the host"""
    t = time.perf_counter()
    S = s.S
    at, out = 0, []
    for n, V in zip(blk, Vs):
        if n < 0:
            at += -n
            continue
        ii, jj = np.tril_indices(n)
        M = np.zeros((n, n))
        w = S[at:at + ii.size] * np.where(ii == jj, 1.0, 0.7071067811865476)
        M[ii, jj] = w
        M[jj, ii] = w
        out.append(M @ V)
        at += ii.size
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
    res = {w: [s.block_multiply(w, f["L"]) for _ in range(REPS + 1)] for w in ("S", "dual")}
    t = time.perf_counter()
    s.block_multiply("S", f["L"])
    call_ms = 1e3 * (time.perf_counter() - t)
    kern = {w: float(np.median([r["ms"] for r in res[w][1:]])) for w in res}
    xs = s.evaluate()["XS"]
    host = float(np.median([host_route(s, blk, f["L"]) for _ in range(4)][1:]))
    ms0 = copy_ms(8 * a.vec_len)
    r0 = res["S"][0]
    print("%-22s blocks %5d vec_len %9d rank sum %6d | iterations %5d, one %.3f ms | block_multiply S %.4f ms (first %.4f), dual %.4f ms (first %.4f), whole call %.3f ms wall | "
          "get_S + smat + product %.2f ms wall | device copy of %d B %.4f ms | S / copy %.2f, dual / copy %.2f, S / iteration %.3f, dual / iteration %.3f, host route / call %.0f | "
          "||S L||_F %.3e, sum <L, S L> %.6e, evaluate <X, S> %.6e"
          % (name, len(blk), a.vec_len, r0["rank_sum"], s.info_iter_num, iter_ms, kern["S"], r0["ms"], kern["dual"], res["dual"][0]["ms"], call_ms, host, 8 * a.vec_len, ms0,
             kern["S"] / ms0, kern["dual"] / ms0, kern["S"] / iter_ms, kern["dual"] / iter_ms, host / call_ms, r0["norm"], r0["inner"], xs), flush=True)
