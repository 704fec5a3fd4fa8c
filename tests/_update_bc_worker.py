"""Worker of tests/test_gpu_update_bc.py::test_two_ranks_in_two_processes: one PROCESS per rank (torch.distributed, gloo over
127.0.0.1), both on GPU 0, the all-reduce hook staged through the host.  pendulum N = 80 sharded by blocks: init, K1 iterations,
cuadmm_update_bC with the perturbed data on every rank (the full b and C, as with init), K2 iterations.  Rank 0 writes the start
of the second stage (X0, y0, S0, sigma) and its info arrays to argv[1]; the test compares them with the oracle."""
import ctypes as C
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
signal.alarm(int(sys.argv[4]))               # this rank's own time limit: a rank that hangs ends itself
import torch
import torch.distributed as dist

import cuadmm_amd
from cuadmm_amd._lib import check
from tests._update_bc_common import INFO, init_with, perturb
from tests.conftest import load_npz_problem
from tests.helpers import problem_to_amd

K1, K2 = int(sys.argv[2]), int(sys.argv[3])
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group(backend="gloo", rank=rank, world_size=world)
lib = cuadmm_amd.load()


def hook(ptr, count, stream):
    check(lib.cuadmm_dev_sync())
    h = np.empty(count)
    check(lib.cuadmm_memcpy_d2h(h.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), count * 8))
    t = torch.from_numpy(h)
    dist.all_reduce(t)
    check(lib.cuadmm_memcpy_h2d(C.c_void_p(ptr), h.ctypes.data_as(C.c_void_p), count * 8))


def whole(s, part, n):
    b0, e0, _, _ = s.shard()
    v = np.zeros(n); v[b0:e0] = part
    t = torch.from_numpy(v); dist.all_reduce(t)
    return v


a = problem_to_amd(load_npz_problem("pendulum_N=80"))
b2, C2 = perturb(a.b_indices, a.b_vals, a.con_num), perturb(a.C_indices, a.C_vals, a.vec_len)
s = cuadmm_amd.SDPSolver(device=0, verbose=False, rank=rank, world=world)
s.set_allreduce(hook)
init_with(s, a, (a.b_indices, a.b_vals), (a.C_indices, a.C_vals))
s.solve(K1, 0.0, 0, 50, 100, 11000, 1.05)
X0, S0, y0, sig = whole(s, s.X, a.vec_len), whole(s, s.S, a.vec_len), s.y, s.state()["sig"]
s.update_bC(b2[0], b2[1], C2[0], C2[1], True, sig)
s.solve(K2, 0.0, 0, 50, 100, 11000, 1.05)
if rank == 0:
    np.savez(sys.argv[1], X0=X0, y0=y0, S0=S0, sig0=sig, shard=np.array(s.shard()), world=world, iters=s.info_iter_num,
             **{k: s.info_arr(k) for k in INFO})
del s
dist.barrier()
dist.destroy_process_group()
