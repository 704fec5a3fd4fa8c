"""cuadmm_update_bC: new b and / or C on a factored solver (include/cuadmm_amd.h; csrc/engine_update.hip, the update kernels in
csrc/vec_kernels.hip).  The contract is "the state cuadmm_init with the new data and the current iterate would have left", and
the engine is bit-reproducible, so the main check is array_equal against a freshly initialised solver.

The perturbed data (tests/_update_bc_common.py: perturb): every nonzero scaled by 1 + 0.05 cos(i), one nonzero dropped, one new
index added -- for b and for C alike.  The synthetic inputs get a thinned b (every 7th entry dropped) and make_synthetic's sparse C,
so that there is an index to add."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd.synthetic import config_c4_blk, make_synthetic
from oracle import cuadmm_oracle as orc
from tests._update_bc_common import INFO, init_with, perturb, snapshot, thin
from tests.conftest import ROOT, load_npz_problem
from tests.helpers import problem_to_amd

pytestmark = pytest.mark.gpu

K1, K2 = 12, 15
SGS, ADMM = 11000, 0
_cache = {}


def problem(name):
    """name -> (cuadmm_amd.Problem, b = (idx, val), C = (idx, val)); built once per module"""
    if name not in _cache:
        if name == "closed":             # C2-like: equal 32 x 32 blocks, every constraint local to one block (closed-block kernels, batches)
            q = make_synthetic([32] * 300, cons_per_block=5, seed=3, dense_C=False)
        elif name == "mixed":            # C4-like: sizes {3, 6, 10, 15, 28, 45}
            q = make_synthetic(config_c4_blk(600, seed=4), cons_per_block=3, seed=4, dense_C=False)
        elif name == "duo":              # two block sizes, block-diagonal: the in-process group with owned constraints
            q = make_synthetic([12] * 40 + [30] * 24, cons_per_block=4, seed=6, dense_C=False)
        elif name == "ublock":
            from tests.test_f4_free_and_rank import _problem_with_free_block
            a = _problem_with_free_block()
            _cache[name] = (a, thin(a.b_indices, a.b_vals), thin(a.C_indices, a.C_vals))
            return _cache[name]
        else:
            a = problem_to_amd(load_npz_problem(name))
            _cache[name] = (a, (a.b_indices, a.b_vals), (a.C_indices, a.C_vals))
            return _cache[name]
        a = cuadmm_amd.Problem(q.vec_len, q.con_num, q.blk, q.At_col_ptrs, q.At_row_ids, q.At_vals, q.b_idx, q.b_vals, q.C_idx, q.C_vals)
        _cache[name] = (a, thin(a.b_indices, a.b_vals), (a.C_indices, a.C_vals))
    return _cache[name]


def perturbed(name):
    a, b, C = problem(name)
    return perturb(b[0], b[1], a.con_num), perturb(C[0], C[1], a.vec_len)


def solver(options=None, **kw):
    return cuadmm_amd.SDPSolver(verbose=False, options=options, **kw)


def solve(s, iters, sw):
    return s.solve(iters, 0.0, 0, 50, 100, sw, 1.05)


def assert_same(u, f, what):
    names = list(INFO) + ["state", "info_iter_num", "X", "y", "S"]
    for nm, va, vb in zip(names, snapshot(u), snapshot(f)):
        assert va.shape == vb.shape and np.array_equal(va, vb), "%s: %s differs (max |d| = %.3e)" % (
            what, nm, float(np.max(np.abs(va - vb))) if va.shape == vb.shape and va.size else -1.0)


def updated_and_fresh(name, sw, new_b=True, new_C=True, keep=True, start_from="self", options=None):
    """U: init(b, C), K1 iterations, update_bC.  F: a fresh init with the new data and U's iterate before the update -- read from U
    itself (which puts U's vectors back into the caller's units first) or from a twin that ran the same K1 iterations (U is then
    updated straight from the scaled state its solve left: the rescaling runs on the device where the y-solve lives there)."""
    a, b, C = problem(name)
    b2, C2 = perturbed(name)
    u = solver(options)
    init_with(u, a, b, C)
    solve(u, K1, sw)
    src = u
    if start_from == "twin":
        src = solver(options)
        init_with(src, a, b, C)
        solve(src, K1, sw)
    X0, y0, S0, sig = (src.X, src.y, src.S, src.state()["sig"]) if keep else (None, None, None, src.state()["sig"])
    u.update_bC(b2[0] if new_b else None, b2[1] if new_b else None, C2[0] if new_C else None, C2[1] if new_C else None, keep, sig)
    f = solver(options)
    init_with(f, a, b2 if new_b else b, C2 if new_C else C, X0, y0, S0, sig)
    return u, f, (X0, y0, S0, sig)


# ---- 1. equivalence with a fresh init, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("sw", [SGS, ADMM], ids=["sGS", "ADMM"])
@pytest.mark.parametrize("name,start_from", [("closed", "self"), ("closed", "twin"), ("mixed", "self"), ("pendulum_N=80", "self"),
                                             ("pendulum_N=80", "twin"), ("PlanarHand_N=1_MOMENT", "self"), ("ublock", "self")])
def test_update_equals_fresh_init(name, start_from, sw):
    u, f, _ = updated_and_fresh(name, sw, start_from=start_from)
    assert_same(u, f, "after the update")              # scaling constants, residual scalars, X / y / S in init's units, empty info arrays
    assert u.info_iter_num == 0 and u.info_arr("pobj").size == 0 and u.total_time == 0.0
    solve(u, K2, sw); solve(f, K2, sw)
    assert_same(u, f, "after %d iterations" % K2)
    assert u.info_arr("pobj").size == K2
    # ... and solve(if_first = 0) continues both alike
    u.solve(5, 0.0, 0, 50, 100, sw, 1.05, if_first=False); f.solve(5, 0.0, 0, 50, 100, sw, 1.05, if_first=False)
    assert_same(u, f, "continued")


@pytest.mark.parametrize("sw", [SGS, ADMM], ids=["sGS", "ADMM"])
@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_cold_update_equals_fresh_cold_init(name, sw):
    u, f, _ = updated_and_fresh(name, sw, keep=False)
    assert_same(u, f, "after the update")
    solve(u, K2, sw); solve(f, K2, sw)
    assert_same(u, f, "after %d iterations" % K2)


@pytest.mark.parametrize("options", [{"fuse": 0}, {"host_solve": 1}, {"l21_device": 2}, {"eig_rank": 3}], ids=["unfused", "host_solve", "hybrid", "eig_rank"])
def test_update_equals_fresh_init_on_the_other_paths(options):
    """unfused iteration; y-solve on the host (y and b live there); the hybrid solve; the rank-limited projection"""
    opts = dict(options)
    kw = {"eig_rank": opts.pop("eig_rank")} if "eig_rank" in opts else {}
    name = "pendulum_N=80" if "l21_device" in opts else "closed"
    a, b, C = problem(name)
    b2, C2 = perturbed(name)
    u, f = solver(opts, **kw), solver(opts, **kw)
    init_with(u, a, b, C)
    solve(u, K1, SGS)
    t = solver(opts, **kw)
    init_with(t, a, b, C)
    solve(t, K1, SGS)
    sig = t.state()["sig"]
    X0, y0, S0 = t.X, t.y, t.S
    u.update_bC(b2[0], b2[1], C2[0], C2[1], True, sig)
    init_with(f, a, b2, C2, X0, y0, S0, sig)
    solve(u, K2, SGS); solve(f, K2, SGS)
    assert_same(u, f, str(options))


# ---- 2. against the oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_updated_solver_against_the_oracle(name):
    """OracleSolver.init(b', C', X0, y0, S0, sig) and K2 iterations.  Tolerances: those of the trajectory tests of the same inputs --
    tests/test_gpu_moment_parity.py (TOL head 1e-8 relative with its ATOL floors) for pendulum, tests/test_gpu_solver.py
    (test_trajectory_vs_oracle_golden: rtol 1e-8, atol 1e-11) for the synthetic input; sigma exact in both."""
    from tests.test_gpu_moment_parity import rel_dev
    from tests.test_gpu_solver import _cmp
    a, _, _ = problem(name)
    b2, C2 = perturbed(name)
    u, _, (X0, y0, S0, sig) = updated_and_fresh(name, SGS)
    solve(u, K2, SGS)
    o = orc.OracleSolver().init(a.vec_len, a.con_num, a.At_csc_col_ptrs, a.At_csc_row_ids, a.At_csc_vals, b2[0], b2[1], C2[0], C2[1],
                                a.blk_vals, X0, y0, S0, sig)
    info = o.solve(K2, 0.0, 0, 50, 100, SGS, 1.05)
    st = u.state()
    assert abs(st["bscale"] - o.bscale) <= 1e-13 * o.bscale and abs(st["Cscale"] - o.Cscale) <= 1e-13 * o.Cscale
    for nm in ("errRp", "errRd", "pobj", "dobj", "relgap"):
        ref = np.array(getattr(info, nm))
        if name.startswith("pendulum"):
            dev = rel_dev(u.info_arr(nm), ref, nm)
            print("%s %s: deviation %.3e" % (name, nm, dev))
            assert dev <= 1e-8, (name, nm, dev)
        else:
            _cmp(name + ":" + nm, u.info_arr(nm), ref, rtol=1e-8, atol=1e-11)
    assert np.array_equal(u.info_arr("sig"), np.array(info.sig))


# ---- 3. only one of the two changes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["b", "C"])
@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_only_one_of_the_two_changes(name, which):
    a, b, C = problem(name)
    u0 = solver()
    init_with(u0, a, b, C)
    st0 = u0.state()
    u, f, _ = updated_and_fresh(name, SGS, new_b=which == "b", new_C=which == "C", start_from="twin")
    st = u.state()
    if which == "C":
        assert st["bscale"] == st0["bscale"] and st["norm_borg"] == st0["norm_borg"] and st["Cscale"] != st0["Cscale"]
    else:
        assert st["Cscale"] == st0["Cscale"] and st["norm_Corg"] == st0["norm_Corg"] and st["bscale"] != st0["bscale"]
    assert_same(u, f, "after the update")
    solve(u, K2, SGS); solve(f, K2, SGS)
    assert_same(u, f, "only %s" % which)


# ---- 4. atomic refusal ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_a_refused_update_leaves_the_solver_as_it_was(name):
    import ctypes as C_
    a, b, C = problem(name)
    b2, C2 = perturbed(name)
    u, twin = solver(), solver()
    for s in (u, twin):
        init_with(s, a, b, C)
        solve(s, K1, SGS)
    bad_b = (np.append(b2[0], a.con_num).astype(np.int32), np.append(b2[1], 1.0))          # out of range
    bad_C = (np.append(C2[0], C2[0][0]).astype(np.int32), np.append(C2[1], 1.0))           # an index twice
    for args in ((bad_b[0], bad_b[1], C2[0], C2[1]), (b2[0], b2[1], bad_C[0], bad_C[1])):
        with pytest.raises(cuadmm_amd.CuadmmError) as e:
            u.update_bC(*args)
        assert e.value.code == -1
    lib = cuadmm_amd.load()
    bi, bv = np.ascontiguousarray(b2[0]), np.ascontiguousarray(b2[1])
    rc = lib.cuadmm_update_bC(u._h, bi.ctypes.data_as(C_.c_void_p), bv.ctypes.data_as(C_.c_void_p), int(bi.size), None, None, 3, 1, 0.0)
    assert rc == -1 and len(lib.cuadmm_last_error()) > 0                                    # C_nnz > 0 with NULL pointers
    u.solve(K2, 0.0, 0, 50, 100, SGS, 1.05, if_first=False); twin.solve(K2, 0.0, 0, 50, 100, SGS, 1.05, if_first=False)
    assert_same(u, twin, "after three refused updates")


# ---- 5. repeated updates --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["closed", "pendulum_N=80"])
def test_five_updates_in_a_row(name):
    """solves between the updates switch from sGS to ADMM at iteration 5 (best-iterate bookkeeping, the closed blocks' batches):
    nothing of an earlier stage may reach the last one"""
    a, b, C = problem(name)
    u = solver()
    init_with(u, a, b, C)
    cur_b, cur_C = b, C
    for stage in range(5):
        u.solve(9, 0.0, 0, 50, 100, 5, 1.05)
        cur_b, cur_C = perturb(cur_b[0], cur_b[1], a.con_num), perturb(cur_C[0], cur_C[1], a.vec_len)
        if stage == 4:
            X0, y0, S0, sig = u.X, u.y, u.S, u.state()["sig"]
        u.update_bC(cur_b[0], cur_b[1], cur_C[0], cur_C[1], True, u.state()["sig"])
    f = solver()
    init_with(f, a, cur_b, cur_C, X0, y0, S0, sig)
    assert_same(u, f, "after the fifth update")
    u.solve(K2, 0.0, 0, 50, 100, 5, 1.05); f.solve(K2, 0.0, 0, 50, 100, 5, 1.05)
    assert_same(u, f, "last stage")


# ---- 6. in-process group --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["duo", "pendulum_N=80"])
def test_in_process_group_forwards_the_update(name):
    """duo_init(device_num_requested = 2, duo_share_device = 1) on a block-diagonal input with two sizes (owned constraints) and on
    pendulum N = 80 (coupled: the replicated y-solve), update through the leader; against a fresh group at the tolerance
    tests/test_gpu_solver.py (test_duo_solver_n_devices_from_one_process) uses between a group and a single engine: 1e-9 / 1e-12."""
    from tests.test_gpu_solver import _cmp
    a, b, C = problem(name)
    b2, C2 = perturbed(name)

    def duo(bb, CC, X0=None, y0=None, S0=None, sig=1.0):
        s = solver({"duo_share_device": 1})
        s.duo_init(True, 2, 15, 30, a.vec_len, a.con_num, a.At_csc_col_ptrs, a.At_csc_row_ids, a.At_csc_vals, a.At_nnz, bb[0], bb[1], len(bb[0]),
                   CC[0], CC[1], len(CC[0]), a.blk_vals, a.mat_num, X0, y0, S0, sig)
        return s
    u = duo(b, C)
    solve(u, K1, SGS)
    assert u.group_info()["engines"] == 2
    X0, y0, S0, sig = u.X, u.y, u.S, u.state()["sig"]
    u.update_bC(b2[0], b2[1], C2[0], C2[1], True, sig)
    f = duo(b2, C2, X0, y0, S0, sig)
    solve(u, K2, SGS); solve(f, K2, SGS)
    assert u.info_iter_num == f.info_iter_num == K2 and u.info_arr("pobj").size == K2
    for nm in ("errRp", "errRd", "pobj", "dobj", "relgap"):
        _cmp("group:" + nm, u.info_arr(nm), f.info_arr(nm), rtol=1e-9, atol=1e-12)
    assert np.array_equal(u.info_arr("sig"), f.info_arr("sig"))
    for va, vb in ((u.X, f.X), (u.y, f.y), (u.S, f.S)):
        assert va.shape == vb.shape and np.max(np.abs(va - vb)) <= 1e-9 * (1 + np.max(np.abs(vb)))
    with pytest.raises(cuadmm_amd.CuadmmError):                # refused by the leader before any rank sees it
        u.update_bC([a.con_num], [1.0])


# ---- 7. two ranks in two processes ----------------------------------------------------------------------------------------
def test_two_ranks_in_two_processes(tmp_path):
    """pendulum N = 80 on two ranks (one process each, both on GPU 0, gloo): the sharded run after an update against the oracle
    started from the same X0, y0, S0, sigma, at the one-rank tolerance of tests/test_gpu_moment_parity.py (TOL head 1e-8, ATOL),
    as tests/test_gpu_sharded_procs.py compares its ranks.  Three processes in all; each rank ends itself after 240 s."""
    from tests.test_gpu_moment_parity import rel_dev
    out = tmp_path / "res.npz"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29661", os.path.join(ROOT, "tests", "_update_bc_worker.py"), str(out), str(K1), str(K2), "240"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d = np.load(out)
    a, _, _ = problem("pendulum_N=80")
    b2, C2 = perturbed("pendulum_N=80")
    assert int(d["world"]) == 2 and d["shard"][0] == 0 and 0 < d["shard"][1] < a.vec_len and int(d["iters"]) == K2
    o = orc.OracleSolver().init(a.vec_len, a.con_num, a.At_csc_col_ptrs, a.At_csc_row_ids, a.At_csc_vals, b2[0], b2[1], C2[0], C2[1],
                                a.blk_vals, d["X0"], d["y0"], d["S0"], float(d["sig0"]))
    info = o.solve(K2, 0.0, 0, 50, 100, SGS, 1.05)
    for nm in ("errRp", "errRd", "pobj", "dobj", "relgap"):
        assert d[nm].size == K2                                  # the first stage's entries are gone, as after an init
        dev = rel_dev(d[nm], np.array(getattr(info, nm)), nm)
        print("two ranks %s: deviation %.3e" % (nm, dev))
        assert dev <= 1e-8, (nm, dev)
    assert np.array_equal(d["sig"], np.array(info.sig))


# ---- 8. command line ------------------------------------------------------------------------------------------------------
def _write_sparse(path, idx, val):
    with open(path, "w") as f:
        for i, v in zip(idx, val):
            f.write("%d 0 %.17g\n" % (int(i), float(v)))


def test_cli_then_stage(tmp_path):
    a, b, C = problem("closed")
    b2, C2 = perturbed("closed")
    d1, d2, d3 = (str(tmp_path / n) + "/" for n in ("stage0", "stage1", "plain"))
    for d in (d1, d2, d3):
        os.makedirs(d)
    for d in (d1, d3):
        with open(d + "blk.txt", "w") as f:
            f.write("".join("s %d\n" % n for n in a.blk_vals))
        with open(d + "con_num.txt", "w") as f:
            f.write("%d\n" % a.con_num)
        cols = np.repeat(np.arange(a.con_num), np.diff(a.At_csc_col_ptrs))
        with open(d + "At.txt", "w") as f:
            for r, c, v in zip(a.At_csc_row_ids, cols, a.At_csc_vals):
                f.write("%d %d %.17g\n" % (int(r), int(c), float(v)))
        _write_sparse(d + "b.txt", *b)
        _write_sparse(d + "C.txt", *C)
    _write_sparse(d2 + "b.txt", *b2)
    _write_sparse(d2 + "C.txt", *C2)
    exe = os.path.join(ROOT, "cuadmm_amd", "lib", "cuadmm_exe")
    js = str(tmp_path / "run.json")
    r = subprocess.run([exe, d1, "--then=" + d2, "--quiet", "--max_iter=40", "--json=" + js], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.exists(js) and os.path.exists(js + ".1")
    # the Python path of the same stages: the CLI's constants (cli_main.cpp), a cold start, the iterate read between the stages
    s = solver()
    s.init_problem(cuadmm_amd.Problem.from_txt(d1), sig=1.0)
    s.solve(40, 1e-3, 0, 50, 100, 5000, 1.05)
    X1 = s.X
    s.update_bC(b2[0], b2[1], C2[0], C2[1], True, 0.0)
    s.solve(40, 1e-3, 0, 50, 100, 5000, 1.05)
    X2 = s.X
    as_written = lambda x: np.array([float("%.32f" % v) for v in x])
    assert np.array_equal(np.loadtxt(d1 + "X_opt.txt"), as_written(X1))
    assert np.array_equal(np.loadtxt(d2 + "X_opt.txt"), as_written(X2))
    assert not np.array_equal(X1, X2)
    # without --then: one X_opt.txt, the first stage's (what the program has always written), and nothing else new
    r = subprocess.run([exe, d3, "--quiet", "--max_iter=40"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(d3)) == ["At.txt", "C.txt", "X_opt.txt", "b.txt", "blk.txt", "con_num.txt"]
    assert open(d3 + "X_opt.txt").read() == open(d1 + "X_opt.txt").read()


# ---- 9. no host trip ------------------------------------------------------------------------------------------------------
def test_update_moves_only_the_sparse_entries_across_pcie():
    """pendulum N = 80, y-solve on the device, profile = 1: across an update the copy class (h2d / d2h, class 4) gains ONE entry, the
    upload of the sparse entries: 12 bytes per entry of b' and C' (index + value) and nothing of length m = 112 028 or L = 131 945."""
    a, b, C = problem("pendulum_N=80")
    b2, C2 = perturbed("pendulum_N=80")
    s = solver(profile=1)
    init_with(s, a, b, C)
    solve(s, K1, SGS)
    assert s.counters()["dev_solve"] in (1.0, 3.0)
    before = s.profile()["copies"]
    s.update_bC(b2[0], b2[1], C2[0], C2[1], True, 0.0)
    after = s.profile()["copies"]
    bound = 12 * (len(b2[0]) + len(C2[0])) + 64            # + the scalars of the stopping test
    grown = after["launches"] - before["launches"]
    print("copies: +%d entries, %.0f bytes (bound %d; 8 m = %d)" % (grown, after["bytes_per_launch"], bound, 8 * a.con_num))
    assert grown <= 1 and after["bytes_per_launch"] <= bound < 8 * a.con_num


# ---- 10. time sanity ------------------------------------------------------------------------------------------------------
def test_update_is_cheaper_than_the_init_it_replaces():
    a, b, C = problem("PushBox_N=30_MOMENT")
    b2, C2 = perturbed("PushBox_N=30_MOMENT")
    s = solver()
    t0 = time.perf_counter()
    init_with(s, a, b, C)
    t_init = time.perf_counter() - t0
    solve(s, 5, SGS)
    t0 = time.perf_counter()
    s.update_bC(b2[0], b2[1], C2[0], C2[1], True, 0.0)
    t_update = time.perf_counter() - t0
    print("PushBox_N=30: init %.3f s, update_bC %.4f s" % (t_init, t_update))
    assert t_update < t_init
    solve(s, 5, SGS)
    assert np.all(np.isfinite(s.info_arr("pobj")))
