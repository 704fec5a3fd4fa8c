"""bench.py's outputs: `--dump-outputs DIR` writes what the timed solve computed (X, y, S after its last step) as float64 .npy files,
long arrays as a fixed seeded sample, and a plain run (no --full) prints the headline figure without the supplementary measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_samples_long_arrays_at_fixed_indices(tmp_path):
    n = bench.DUMP_MAX_ELEMS + 12345
    a = np.arange(n, dtype=np.float64)
    bench.dump_outputs(str(tmp_path / "a"), {"X": a, "y": np.arange(7, dtype=np.float32)})
    bench.dump_outputs(str(tmp_path / "b"), {"X": -a})
    xa, xb = np.load(tmp_path / "a" / "X.npy"), np.load(tmp_path / "b" / "X.npy")
    assert xa.dtype == np.float64 and xa.size == bench.DUMP_MAX_ELEMS
    assert np.array_equal(xa, -xb)                            # the same indices in every run
    assert np.all(np.diff(xa) > 0) and xa[-1] < n             # sorted, distinct elements of the array
    y = np.load(tmp_path / "a" / "y.npy")
    assert y.dtype == np.float64 and np.array_equal(y, np.arange(7))   # short arrays in full


def test_dump_of_the_headline_workload_stays_below_64_mb(tmp_path):
    L = bench.BLOCKS_PER_GPU * bench.BLOCK_N * (bench.BLOCK_N + 1) // 2     # svec length of X and S of the default workload
    bench.dump_outputs(str(tmp_path), {"X": np.zeros(L), "y": np.zeros(5 * bench.BLOCKS_PER_GPU), "S": np.zeros(L)})
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 20


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs_are_the_timed_solves(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--blocks-per-gpu", "600", "--steps", "12",
                        "--warmup", "3", "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 12 and d["warmup"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-9 * 1e3     # one GPU: value = steps / time, ms_per_step = time / steps
    for k in ("steady_state", "with_checkpoint", "pcie_inclusive", "breakdown_ms_per_iter", "y_solve", "time_to_tol", "cpu_baseline"):
        assert k not in d, k

    # the same warm-up and timed solve in this process
    import cuadmm_amd
    from cuadmm_amd import synthetic
    p = synthetic.make_synthetic([bench.BLOCK_N] * 600)
    s = cuadmm_amd.SDPSolver(device=0, verbose=False, profile=2, psd_steps=True)
    s.init_problem(cuadmm_amd.Problem(p.vec_len, p.con_num, p.blk, p.At_col_ptrs, p.At_row_ids, p.At_vals, p.b_idx, p.b_vals,
                                      p.C_idx, p.C_vals))
    s.solve(3, 0.0, 0, 50, 100, 0, 1.05)
    s.solve(12, 0.0, 0, 50, 100, 0, 1.05, if_first=False)
    for name, ref in (("X", s.X), ("y", s.y), ("S", s.S)):
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == ref.shape, name
        assert np.max(np.abs(got - ref)) <= 1e-12 * (1 + np.max(np.abs(ref))), name
