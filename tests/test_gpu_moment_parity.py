"""The moment-relaxation inputs against the ORACLE at a stated tolerance.

PlanarHand_N=1, pendulum N=80, PushT_N=10 and PushT_N=30 are the inputs on which the engine's GPU tail of the A A^T factor
(tail_solve.hip, an explicit inverse), the device-side leading sweeps (lead_solve.hip), the long-row A^T y path and the un-fused
iteration run TOGETHER.  tests/golden/oracle_traj_moment.json (tests/golden/make_traj_moment.py, CPU, dev container) holds the
oracle's per-iteration (errRp, errRd, pobj, dobj, relgap, sig) -- exact sparse solve + LAPACK dsyevd restating
src/solver.cu:478-500,534-647,693-729 -- for the first 60 iterations and at one late checkpoint.  The default engine must
reproduce them to the tolerances below (relative, with an absolute floor of 1e-11 at the roundoff level; sigma exact).

Measured (profiles/r03_moment_parity.log): first 60 iterations <= 7e-9 (PlanarHand, with the 17 152-column GPU tail and the
device-side sweeps: <= 2e-10), late checkpoints <= 3e-8 -- with ONE exception, pobj of PushT_N=30 (27 136-column tail), stated at
POBJ_HEAD_TOL below.  Tolerances: 1e-8 on the head -- the same as every other trajectory test -- and 1e-7 at the late checkpoint
(iteration 200 ... 1000).  One absolute
floor differs: errRp right after an sGS half step is the rounding error of the y-solve itself (1e-12 in the oracle's SuperLU,
up to 1e-10 through the tail's explicit inverse), so its absolute tolerance is 1e-9 -- six orders below any stopping
tolerance; the other quantities carry the usual 1e-11.  y is not compared: A A^T is numerically singular on these inputs (only A^T y is determined)."""
import gzip
import json
import os
import shutil

import numpy as np
import pytest

import cuadmm_amd
from oracle import cuadmm_oracle as orc
from tests.conftest import GOLDEN, load_npz_problem
from tests.helpers import problem_to_amd

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "oracle_traj_moment.json")) as f:
    TRAJ = json.load(f)

SIX = ("errRp", "errRd", "pobj", "dobj", "relgap")
# key -> (head tolerance, late tolerance)
TOL = {key: (1e-8, 1e-7) for key in TRAJ}
# The whole run of examples/pendulum/N=80_licols.log: 100 000 iterations (round 5; 92 minutes of the numpy oracle on eight cores).  Rounding
# differences grow along a nonlinear iteration of that length: at its end the engine agrees with the oracle to 1.1e-5 in errRd and to 1e-9 in
# the objectives (measured, profiles/r05_pendulum_100k.log) -- the oracle itself is 24 % (errRd), 11 % (relgap), 2 % (errRp) away from the row the
# reference printed there, which is what two fp64 implementations of the reference's arithmetic can be expected to share after 100 000 steps.
TOL["pendulum_N=80/switch=11000/late=100000"] = (1e-8, 1e-4)
# pobj of two inputs, stated -- and what it is, since round 6 (profiles/r06_tail_refine.log, r06_tail_pivot.log; DESIGN.md section 2, NOTEBOOK.md "Round 6").
# Rounds 3 - 5 applied the tail as the explicit inverse of an UNPIVOTED factor: accurate to u cond(L22), and L22 carries columns of size 1 / sqrt(pivot) where
# the Schur complement of a large moment relaxation is nearly singular -- 1.1e-7 on PushT_N=30, 8.5e-8 on PushBox_N=50 at an 8 448-column tail (3.8e-9 at the
# planner's 8 192: luck).  Since round 6 the tail's dense LDL^T pivots on the diagonal (option tail_pivot, default): bounded L, accurate inverse at no cost per
# solve -- PushBox_N=50 <= 1.0e-10 at every cut (its oracle solves with SuperLU's pivoted LU).  What remains on the two inputs below is the ORACLE's share: SuperLU
# cannot hold their factors, so their golden y-solves came from the library's unpivoted host LDL^T, whose own division by near-zero pivots is in the golden digits
# (the same factor code on both sides, tail_k = 0, agrees to 9.7e-9 only; the unpivoted tail with one refinement step per triangular solve -- which reproduces that
# arithmetic's order -- to 4.1e-9).  Every other quantity of every input <= 2.3e-9.
POBJ_HEAD_TOL = {"PushT_N=30_MOMENT/switch=11000": 5e-8,        # measured 2.7e-8 (rounds 3 - 5, unpivoted tail: 1.1e-7 ... 4.1e-7 at 3e-7 ... 1e-6)
                 "PlanarHand_N=10_MOMENT/switch=11000": 3e-8}   # measured 1.4e-8 (5.8e-11 at the late checkpoint), with and without pivoting / refinement

# |got - ref| <= tol * |ref| + ATOL: the absolute part is the roundoff floor of the quantity (1e-11, as in the other trajectory tests;
# errRp: the y-solve's own rounding error, see above)
ATOL = {"errRp": 1e-9, "errRd": 1e-11, "pobj": 1e-11, "dobj": 1e-11, "relgap": 1e-11}


def rel_dev(got, ref, nm):
    """deviation in units of the relative tolerance: max(|got - ref| - ATOL, 0) / |ref| (0 where the absolute floor covers it)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    return float(np.max(np.maximum(np.abs(got - ref) - ATOL[nm], 0.0) / np.maximum(np.abs(ref), 1e-300)))


def load_problem(name, tmp_path):
    d = os.path.join(GOLDEN, "problems", name)
    if os.path.isdir(d):
        for fn in os.listdir(d):
            with gzip.open(os.path.join(d, fn), "rb") as f, open(os.path.join(str(tmp_path), fn[:-3]), "wb") as g:
                shutil.copyfileobj(f, g)
        return orc.load_problem_txt(str(tmp_path) + "/")
    return load_npz_problem(name)


def deviations(s, rec):
    """max relative deviation over the head, at the late checkpoint, and whether sigma agrees exactly"""
    head = int(rec["iters"])
    late = int(rec["late"])
    dev_head, dev_late = {}, {}
    for nm in SIX:
        got = s.info_arr(nm)
        ref = np.array([float(x) for x in rec[nm]])
        dev_head[nm] = rel_dev(got[:head], ref, nm)
        r = float(rec["late_" + nm])
        dev_late[nm] = rel_dev(got[late - 1], r, nm)
    sig_ok = np.array_equal(s.info_arr("sig")[:head], np.array([float(x) for x in rec["sig"]])) and \
        s.info_arr("sig")[late - 1] == float(rec["late_sig"])
    return dev_head, dev_late, bool(sig_ok)


def run_and_compare(key, tmp_path, options, pobj_head_tol):
    rec = TRAJ[key]
    p = load_problem(rec["problem"], tmp_path)
    s = cuadmm_amd.SDPSolver(verbose=False, options=options)
    s.init_problem(problem_to_amd(p))
    prm = rec["params"]
    s.solve(int(rec["late"]), 0.0, prm["sig_update_threshold"], prm["sig_update_stage_1"], prm["sig_update_stage_2"],
            prm["switch_admm"], prm["sigscale"])
    dev_head, dev_late, sig_ok = deviations(s, rec)
    c = s.counters()
    print(key, "tail_k", c["tail_k"], "dev_solve", c["dev_solve"], "head", dev_head, "late", dev_late, "sig", sig_ok)
    if not options and rec["problem"] == "pendulum_N=80":
        assert c["tail_k"] > 0 and c["dev_solve"] == 3          # round 6: a 7 168-column tail behind dense tree tops (rounds 3 - 5: 10 496 columns, plain sweeps)
    if not options and rec["problem"] == "PlanarHand_N=1_MOMENT":
        assert c["tail_k"] > 0 and c["dev_solve"] == 3          # round 5: a smaller tail behind dense tree tops (round 4: 17 152 columns, plain sweeps)
    if not options and rec["problem"] == "PushT_N=30_MOMENT":
        assert c["tail_k"] > 0                                  # GPU tail between host-side leading sweeps
    if not options and rec["problem"] in ("PushBox_N=30_MOMENT", "PushBox_N=50_MOMENT"):
        assert c["dev_solve"] == 3                              # round 5: dense tree tops at the small tail (round 4: a larger tail made the forest shallow)
    if options and options.get("lead_tops") == 0 and rec["problem"] in ("PushBox_N=30_MOMENT", "PlanarHand_N=1_MOMENT"):
        assert c["dev_solve"] == 1                              # round 4's plan: the larger tail, plain sweeps
    if not options and rec["problem"] == "PlanarHand_N=10_MOMENT":
        assert c["dev_solve"] == 3                              # round 5: the deep forest cut at height 32, dense tree tops (lead_solve.h); round 4: hybrid
    if options and options.get("l21_device") == 2:
        assert c["dev_solve"] == 2
    assert sig_ok
    th, tl = TOL[key]
    for nm in SIX:
        assert dev_head[nm] <= (pobj_head_tol if nm == "pobj" and pobj_head_tol else th), (nm, dev_head)
        assert dev_late[nm] <= tl, (nm, dev_late)
    # X and S at the late checkpoint (y is not unique on these inputs: A A^T is numerically singular, only A^T y is determined)
    for v, nm in ((s.X, "late_X_norm"), (s.S, "late_S_norm")):
        r = float(rec[nm])
        assert abs(np.linalg.norm(v) - r) <= 10 * tl * (1 + r), nm
    return s


@pytest.mark.parametrize("key", sorted(TRAJ))
def test_moment_relaxation_trajectory_matches_the_oracle(key, tmp_path, ref_logs):
    s = run_and_compare(key, tmp_path, None, POBJ_HEAD_TOL.get(key))
    if key.endswith("/late=100000"):
        # examples/pendulum/N=80_licols.log runs its full 100 000 iterations (stop_tol 1e-6 is never reached); the same run against the
        # last row the REFERENCE printed: two fp64 implementations of a 100 000-step nonlinear iteration share the digits its own
        # contraction preserves -- residuals to ~30 %, objectives to 3 - 4 digits (the oracle itself is 24 % / 11 % / 2 % away from that row
        # in errRd / relgap / errRp).  (Rounds 2 - 5 ran these 100 000 iterations twice: here and in tests/test_gpu_longrun.py.)
        row = ref_logs["pendulum_N=80/sGS"]["rows"][-1]
        assert s.info_iter_num == 100000 == int(row[0])
        for name, col, rel in (("pobj", 3, 1e-3), ("dobj", 4, 1e-3), ("errRp", 1, 0.3), ("errRd", 2, 0.3), ("relgap", 5, 0.3)):
            w = float(row[col])
            assert abs(s.state()[name] - w) <= rel * abs(w), (name, s.state()[name], w)


@pytest.mark.parametrize("tail_k", [8192, 8448, 8704])
def test_parity_does_not_depend_on_where_the_tail_is_cut(tail_k, tmp_path):
    """Parity on nearly singular Schur complements as a property of the SOLVE, not of where the planner's cost model cuts: PushBox_N=50 at the
    planner's 8 192 columns and at the two neighbouring cuts where the unpivoted explicit inverse of rounds 3 - 5 left 8.5e-8 / 4.0e-8 in the primal objective
    (which of the 9 301 pivots at 1e-15 ... 1e-13 the tail held decided).  With the tail's LDL^T pivoted on the diagonal (the default) every quantity holds the
    common 1e-8 at every cut -- measured <= 1.0e-10 -- and the explicit inverse's own residual || z - L (W z) || is 2e-14 instead of 9e-12.  The contract being
    met: the reference's exact LDL^T solve, include/cuadmm/cholesky_cpu.h:89-155 with eps = 1e-15 at src/solver.cu:94."""
    s = run_and_compare("PushBox_N=50_MOMENT/switch=11000", tmp_path, {"tail_k": tail_k}, None)
    ti = s.tail_info()
    assert ti["tail_k"] == tail_k and 0.0 < ti["inverse_residual"] <= 1e-12
    for nm in SIX:                                            # well inside the tolerance, not at its edge
        assert rel_dev(s.info_arr(nm)[:60], np.array([float(x) for x in TRAJ["PushBox_N=50_MOMENT/switch=11000"][nm]]), nm) <= 2e-9, nm


@pytest.mark.parametrize("key,options,pobj_tol", [("PushBox_N=50_MOMENT/switch=11000", {"tail_k": 8448, "tail_pivot": 0}, None),
                                                  ("PushT_N=30_MOMENT/switch=11000", {"tail_pivot": 0}, None)])
def test_refined_unpivoted_tail_reproduces_the_oracle(key, options, pobj_tol, tmp_path):
    """The accuracy mode that found the cause (option tail_refine: one refinement step of each triangular solve against the factor itself, u <- u + W (z - L u),
    x <- x + W^T (v - L^T x)) on the UNPIVOTED factor of rounds 3 - 5: every quantity at 1e-8 where the plain explicit inverse leaves 8.5e-8 (PushBox_N=50 at
    8 448 columns) and 1.1e-7 (PushT_N=30).  Measured 3.6e-11 / 4.1e-9.  Six times the tail's bytes per solve: kept as an option, not the default."""
    s = run_and_compare(key, tmp_path, dict(options, tail_refine=1), pobj_tol)
    ti = s.tail_info()
    assert ti["refined"] and ti["inverse_residual"] > 1e-13      # the unpivoted inverse is the inaccurate one (pivoted: ~2e-14); the refinement repairs the solve


@pytest.mark.parametrize("key", ["PlanarHand_N=1_MOMENT/switch=0", "PushBox_N=30_MOMENT/switch=11000"])
def test_round4_plan_without_tree_tops_still_matches_the_oracle(key, tmp_path):
    """option lead_tops = 0: the planner and the solve of round 4 (a larger tail, plain level-by-level sweeps) -- the same oracle trajectory"""
    run_and_compare(key, tmp_path, {"lead_tops": 0}, POBJ_HEAD_TOL.get(key))


@pytest.mark.skipif(os.environ.get("CUADMM_LONG_TESTS") != "1", reason="125 s of host factorisation (58 M nonzeros on the box's CPUs): run with "
                    "CUADMM_LONG_TESTS=1 (profiles/r06_gpu_tests_long.log); the default suite stays inside the driver's time limit")
def test_pusht30_with_the_factor_on_the_host_is_exact(tmp_path):
    """The same input without the GPU tail: 1e-8 on every quantity (what POBJ_HEAD_TOL above is measured against).
    What this does and does not prove: the oracle trajectory of this input took its y-solves from the library's own host LDL^T
    (SuperLU cannot hold the factor), so with tail_k = 0 both sides solve with the SAME factor -- agreement here shows that the
    engine's iteration AROUND the solve (scaling, projection, updates, residuals) is the oracle's, not that the factor is right.
    The factor is pinned independently: every y the generator used is checked with scipy matvecs alone (relative residual recorded
    per solve in oracle_traj_moment.json, asserted <= 1e-10 by tests/test_oracle_pinning.py::test_host_factor_solves_of_the_large_
    trajectories_were_verified_by_scipy), and cuadmm_aat_* is compared with scipy's SuperLU where SuperLU holds the matrix
    (PushBox_N=30, m = 154 256: test_host_factor_against_superlu)."""
    # every quantity at 1e-8; pobj measured 9.7e-9 since round 4's ordering (1.9e-9 with round 3's): 3e-8 stated for it alone
    run_and_compare("PushT_N=30_MOMENT/switch=11000", tmp_path, {"tail_k": 0}, 3e-8)


def test_pushbox30_hybrid_solve_with_l21_on_the_device_matches_the_oracle(tmp_path):
    """The hybrid y-solve (lead_solve.h: host sweeps over L11, L21 products and the tail on the device) forced on PushBox_N=30 at the
    HOST optimum of the tail size (10 240 columns: forest 1 135 levels deep, the case the mode exists for) -- the same oracle
    trajectory at the same tolerance as the default plan."""
    run_and_compare("PushBox_N=30_MOMENT/switch=11000", tmp_path, {"tail_k": 10240, "l21_device": 2}, None)


def test_pushbox30_host_sweeps_and_hybrid_agree(tmp_path):
    """the same input with the whole leading part on the host (l21_device = 0) and in hybrid mode: iterates agree to the rounding of
    the differently associated L21 sums"""
    p = load_problem("PushBox_N=30_MOMENT", tmp_path)
    out = []
    for opt, mode in (({"tail_k": 10240, "l21_device": 0, "lead_tops": 0}, 0), ({"tail_k": 10240, "l21_device": 2}, 2)):
        s = cuadmm_amd.SDPSolver(verbose=False, options=opt)
        s.init_problem(problem_to_amd(p))
        s.solve(40, 0.0, 0, 50, 100, 20, 1.05)
        assert s.counters()["dev_solve"] == mode and s.counters()["tail_k"] == 10240
        out.append({nm: s.info_arr(nm).copy() for nm in SIX})
    for nm in SIX:
        assert rel_dev(out[1][nm], out[0][nm], nm) <= 1e-8, nm


@pytest.mark.parametrize("name", ["pendulum_N=80", "PlanarHand_N=1_MOMENT"])
def test_resident_and_streaming_leading_sweeps_agree_bit_for_bit(name, tmp_path):
    """lead_solve.hip: the sweeps with a tree's whole stream resident in LDS (small trees: one wavefront; big trees: four, on a
    side stream) and the streaming kernels of round 2 (option lead_stream = 1) gather in the same order with the same group
    sums -- identical iterates, bit for bit."""
    p = load_problem(name, tmp_path)
    out = []
    for opt in ({"lead_tops": 0}, {"lead_tops": 0, "lead_stream": 1}):
        s = cuadmm_amd.SDPSolver(verbose=False, options=opt)
        s.init_problem(problem_to_amd(p))
        s.solve(40, 0.0, 0, 50, 100, 20, 1.05)
        assert s.counters()["dev_solve"] == 1
        out.append((s.info_arr("pobj").copy(), s.info_arr("errRp").copy(), s.y.copy(), s.X.copy()))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name,level", [("pendulum_N=80", 6), ("PlanarHand_N=1_MOMENT", 6), ("PlanarHand_N=1_MOMENT", 20)])
def test_dense_tree_tops_agree_with_the_plain_sweeps(name, level, tmp_path):
    """lead_solve.h, dense tree tops: the leading forest cut at height `level` (option lead_tops; the automatic choice only cuts forests
    the sweeps cannot run), the tops solved through explicit inverses of their diagonal blocks -- the same iterates as the plain
    level-by-level sweeps up to the rounding of the differently associated sums."""
    p = load_problem(name, tmp_path)
    out = []
    k = {"pendulum_N=80": 10496, "PlanarHand_N=1_MOMENT": 17152}[name]        # the same tail on both sides: round 4's plan
    for opt, mode in (({"tail_k": k, "lead_tops": 0}, 1), ({"tail_k": k, "lead_tops": level}, 3), ({"tail_k": k, "lead_tops": level, "lead_stream": 1}, 3)):
        s = cuadmm_amd.SDPSolver(verbose=False, options=opt)
        s.init_problem(problem_to_amd(p))
        s.solve(60, 0.0, 0, 50, 100, 30, 1.05)
        assert s.counters()["dev_solve"] == mode and s.counters()["tail_k"] == k
        out.append(({nm: s.info_arr(nm).copy() for nm in SIX}, s.X.copy(), s.S.copy()))
    for nm in SIX:
        assert rel_dev(out[1][0][nm], out[0][0][nm], nm) <= 1e-8, nm
        assert np.array_equal(out[1][0][nm], out[2][0][nm]), nm        # resident and streaming sweeps of the cut forest: bit for bit
    for a, b in ((out[0][1], out[1][1]), (out[0][2], out[1][2])):
        assert np.linalg.norm(a - b) <= 1e-8 * (1 + np.linalg.norm(a))


def test_a_cut_above_every_tree_falls_back_to_the_plain_sweeps(tmp_path):
    """lead_tops = 500 on pendulum N = 80 (forest 28 levels deep at a 10 496-column tail): no node is that high, there is nothing to cut -- the plain
    sweeps run (counter 1) and the iterates are those of lead_tops = 0, bit for bit."""
    p = load_problem("pendulum_N=80", tmp_path)
    out = []
    for opt in ({"tail_k": 10496, "lead_tops": 0}, {"tail_k": 10496, "lead_tops": 500}):      # (round 4's tail: the planner's own pick has tree tops since round 6)
        s = cuadmm_amd.SDPSolver(verbose=False, options=opt)
        s.init_problem(problem_to_amd(p))
        s.solve(30, 0.0, 0, 50, 100, 15, 1.05)
        assert s.counters()["dev_solve"] == 1
        out.append((s.info_arr("pobj").copy(), s.y.copy(), s.X.copy()))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def test_wide_forest_plan_agrees_with_the_host_solve(tmp_path):
    """bqp-r1-40-1 (m = 269 001, a factor of 0.8 M nonzeros: no dense tail pays): round 5's planner puts a 1 024-column tail in front of the
    device-side sweeps -- 102 000 micro trees on one thread each, the rest cut at height 32 -- instead of the host solve of rounds 1 - 4
    (option lead_tops = 0).  The same iterates to the rounding of the differently associated sums."""
    p = load_problem("bqp-r1-40-1", tmp_path)
    out = []
    for opt, mode, k in (({"lead_tops": 0}, 0, 0), ({}, 3, 1024)):
        s = cuadmm_amd.SDPSolver(verbose=False, options=opt)
        s.init_problem(problem_to_amd(p))
        s.solve(60, 0.0, 0, 50, 100, 30, 1.05)
        c = s.counters()
        assert c["dev_solve"] == mode and c["tail_k"] == k
        out.append(({nm: s.info_arr(nm).copy() for nm in SIX}, s.X.copy(), s.y.copy()))
    for nm in SIX:
        assert rel_dev(out[1][0][nm], out[0][0][nm], nm) <= 1e-8, nm
    for i in (1, 2):
        assert np.linalg.norm(out[0][i] - out[1][i]) <= 1e-8 * (1 + np.linalg.norm(out[0][i]))
