"""The closed-block iteration (psd_sign_closed.h) on the hand-placed problems of tests/_closed_cases.py: the FULL instantiations
for n = 16, 48 and 64 (a class made only of blocks that fill their tile, PsdRange::full) and the shapes of a block's record
that make_synthetic never produces -- eight scatter rounds, nonzeros on the first and the last (diagonal) slot, blocks with
different numbers of rows or none, rows of length 1 beside one of 57, eight rows and 64 nonzeros together.

Every case runs 12 iterations with stop_tol = 0 in three phases (switch_admm = 0: ADMM only; 5: sGS then the switch; 1000: sGS
only, the kernel's mode 1) four times:

    a   batch = 0                    one launch per iteration: psd_sign_closed_kernel<NT, OCC, FULL>
    b   batch = 16, batch_mixed = 1  several iterations per launch: psd_sign_closed_cu_kernel<NT, WAVES, OCC, FULL, false>
    c   fuse_solve = 0               the stand-alone y-solve and statistics kernels, no closed blocks
    o   the numpy oracle

a = b to the bit; a against c and a against o at the bounds of tests/test_gpu_fused.py (test_closed_blocks_solve_for_their_own_
multipliers, test_fused_iteration_vs_oracle), with X and S against the oracle taken PER BLOCK, so that one wrong block cannot hide
behind the largest entry of the problem.

A block without rows (the rowless cases) stays in the closed path: init_matrices gives it a local-row descriptor with zero rows,
init_closed a record with nk = nnz = nrounds = maxlen = 0 (zero factor, D = 1), and the kernel skips the solve (nk > 0), runs no
scatter round and no row sum; the block's projection and its S / X updates still run inside the closed kernel.

Which instantiations a case launches (launch_sign_wave, PsdPlan::project; FULL only where the whole range has n = 16 NT):
    *-16     NT = 1, OCC = 8, FULL      dense-48  NT = 3, OCC = 2, FULL      *-edges  NT = 1, 2, 3, 4, none FULL
    *-32     NT = 2, OCC = 4 (3), FULL  dense-64  NT = 4, OCC = 1, FULL

Every test prints its worst error / bound ratios (pytest -s).  On record from an MI355X, the largest over the three phases:
against c at most 3.8e-4 of the bound on the info arrays (ragged-32) and 1.3e-3 on X / y / S (ragged-edges); against the oracle
at most 9.4e-5 on the info arrays (ragged-edges), 1.7e-6 on a block of X (ragged-16), 3.3e-6 on a block of S (dense-edges) and
5.2e-6 on y (ragged-edges).  The borrowed bounds are three to six orders wider than what the kernels leave; they still separate
a wrong number from a right one: zeroing the scatter's rounds >= 2 fails the nine stacked tests, the 1/sqrt(2) factor on a diagonal
slot of the first walk fails all 45, dropping row 7 from b^T y fails the 30 tests with ADMM iterations (sw = 0, 5).
"""
import numpy as np
import pytest

import cuadmm_amd
from oracle import cuadmm_oracle as orc
from tests import _closed_cases as cc

pytestmark = pytest.mark.gpu

INFO = ("errRp", "errRd", "pobj", "dobj", "relgap")
ITERS = 12
OCC3 = {"psd_w32_occ": 3, "psd_cu_occ": 3}          # three wavefronts per SIMD: psd_sign_closed_kernel<2, 3, .>, ..._cu_kernel<2, 12, 3, .>

PARAMS = [pytest.param(name, sw, {}, id="%s-sw%d" % (name, sw)) for name in sorted(cc.CASES) for sw in (0, 5, 1000)] + \
         [pytest.param("dense-32", sw, OCC3, id="dense-32-occ3-sw%d" % sw) for sw in (0, 5, 1000)]

_oracle = {}


def _oracle_run(name, sw):
    """the reference trajectory of (case, phase): computed once, shared, never written to"""
    if (name, sw) not in _oracle:
        o = orc.OracleSolver().init_problem(orc.Problem(*cc.case(name)))
        info = o.solve(ITERS, 0.0, 0, 50, 100, sw, 1.05)
        _oracle[(name, sw)] = ({nm: np.asarray(getattr(info, nm), float) for nm in INFO}, o.X.copy(), o.y.copy(), o.S.copy())
    return _oracle[(name, sw)]


def _run(name, sw, options):
    args = cc.case(name)
    opts = dict(options)
    if int(np.max(args[2])) > 32:
        opts["psd_wave4_min"] = 1                    # the one-wavefront kernels for 32 < n <= 64 whatever the count
    s = cuadmm_amd.SDPSolver(verbose=False, options=opts)
    s.init_problem(cuadmm_amd.Problem(*args))
    s.solve(ITERS, 0.0, 0, 50, 100, sw, 1.05)
    assert s.info_iter_num == ITERS
    return s


def _info_ratio(got, ref, rtol, atol):
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))


def _vec_ratio(got, ref, tol):
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref)) / (tol * (1 + np.max(np.abs(ref)))))


def _block_ratio(got, ref, blk, tol):
    """max over blocks k of  max|got_k - ref_k| / (tol (1 + max|ref_k|))"""
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    b64 = blk.astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(b64 * (b64 + 1) // 2)])[:-1]
    err = np.maximum.reduceat(np.abs(got - ref), starts)
    mag = np.maximum.reduceat(np.abs(ref), starts)
    return float(np.max(err / (tol * (1 + mag))))


@pytest.mark.parametrize("name,sw,env", PARAMS)
def test_closed_iteration_on_hand_placed_blocks(name, sw, env):
    blk = cc.case(name)[2]
    a = _run(name, sw, dict(env, batch=0))
    b = _run(name, sw, dict(env, batch=16, batch_mixed=1))
    c = _run(name, sw, dict(env, fuse_solve=0))
    ca, cb, cx = a.counters(), b.counters(), c.counters()
    assert ca["closed_blocks"] == 1 and cb["closed_blocks"] == 1 and cx["closed_blocks"] == 0
    assert ca["batch_launches"] == 0
    if sw == 0:
        assert cb["batch_launches"] >= 1
    aX, ay, aS = a.X, a.y, a.S
    # a = b: the batched launches leave the same bits
    for nm in INFO + ("sig",):
        assert np.array_equal(a.info_arr(nm), b.info_arr(nm)), nm
    assert np.array_equal(aX, b.X) and np.array_equal(ay, b.y) and np.array_equal(aS, b.S)
    ratios = {}
    # a against c: the block's own solve and row sums against the stand-alone kernels
    ratios["c.info"] = max(_info_ratio(a.info_arr(nm), c.info_arr(nm), 1e-10, 1e-12) for nm in INFO)
    ratios["c.XyS"] = max(_vec_ratio(aX, c.X, 1e-11), _vec_ratio(ay, c.y, 1e-11), _vec_ratio(aS, c.S, 1e-11))
    # a against the oracle
    oinfo, oX, oy, oS = _oracle_run(name, sw)
    ratios["o.info"] = max(_info_ratio(a.info_arr(nm), oinfo[nm], 1e-8, 1e-11) for nm in INFO)
    ratios["o.X_blk"] = _block_ratio(aX, oX, blk, 1e-8)
    ratios["o.S_blk"] = _block_ratio(aS, oS, blk, 1e-8)
    ratios["o.y"] = _vec_ratio(ay, oy, 1e-8)
    print("closed-edges %s sw=%d%s: worst error / bound: %s" % (name, sw, " occ3" if env else "", "  ".join("%s %.3g" % kv for kv in ratios.items())))
    assert np.array_equal(a.info_arr("sig"), c.info_arr("sig"))
    for what, r in ratios.items():
        assert r <= 1.0, (what, r)
