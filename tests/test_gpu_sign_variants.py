"""GPU parity of EVERY launch variant of the batched-GEMM sign path (csrc/psd_large.hip, n > 64) against the oracle (LAPACK), on the spectra
families that stress the schedule.  The default options only ever select a few of the instantiations for the sizes the other tests
use (the one-launch kernel on 32-wide tiles below n = 641; the 64-wide mirrored GEMM and the decision kernel on N(0, 1) input at
n >= 2000 only); here each one is forced through cuadmm_op_psd_project_opts -- options from the built-in defaults, never the environment
-- at the smallest shapes that reach it.  tests/test_sign_groups_host.py proves on the CPU that every (blk, opts) pair below
(tests/helpers.py: SIGN_*) gets the variant it names.

Reference: orc.psd_project_svec.  Tolerance: that of test_project_sign_path_spectra, 2e-12 * max(||M||_2, 1e-300) * sqrt 2 per block.
psd_lg_cluster_wgs is never raised here: the one-launch kernel's barriers rely on a co-resident grid.

Step counts of one run on an MI355X are in NOTEBOOK.md ("Sign path: step counts of the variant tests"); the parity test below prints
them (pytest -s)."""
import numpy as np
import pytest

import cuadmm_amd
from oracle import cuadmm_oracle as orc
from tests import helpers as H
from tests.helpers import block_scale, plan_matrix, psd_project_gpu

pytestmark = pytest.mark.gpu

KINDS = H.FAMILIES + ("zero", "tail")         # randn, lowrank, graded, psd, nsd, clustered, moment (rank 3 + noise at 1e-12, ~40 steps)
_INPUTS, _RUNS = {}, {}
# extra seed words, chosen with the schedule's host model (cuadmm_sign_sched_simulate, lagged, on |eigenvalues| / ||M||_1) so that a
# variant with few cases still ends in both buffers (test_multi_launch_variant_ends_in_both_buffers)
_SEED_SALT = {((800,), ("graded",)): 2}


TAIL_HEAD = 704          # = 22 x 32: the tiles of columns >= 704 own the slots 253 ... of a member on 32-wide tiles


def tail_matrix(n, rng):
    """block diagonal: rows < 704 hold a spectrum the sign iteration resolves in a few steps (+-1, 2), the rows from 704 on a graded one
    (both signs over 14 decades, ~46 steps).  Everything still unresolved then sits in tiles whose statistics slots are 256 and above --
    the second trip of lg_reduce_decide's slot loop: a decision that misses them stops ~30 steps early."""
    from tests.test_gpu_psd import _spectrum_matrix
    Q, _ = np.linalg.qr(rng.standard_normal((TAIL_HEAD, TAIL_HEAD)))
    M = np.zeros((n, n))
    M[:TAIL_HEAD, :TAIL_HEAD] = (Q * rng.choice([1.0, -1.0, 2.0], TAIL_HEAD)) @ Q.T
    M[TAIL_HEAD:, TAIL_HEAD:] = _spectrum_matrix(n - TAIL_HEAD, "graded", rng)
    return (M + M.T) / 2


def inputs(blk, kinds):
    """one matrix per block (block k of family kinds[k], scaled by block_scale(k)), the packed vector and the oracle's projection: made once"""
    key = (tuple(blk), tuple(kinds))
    if key not in _INPUTS:
        rng = np.random.default_rng([len(blk), int(sum(blk))] + [KINDS.index(k) for k in kinds] + [_SEED_SALT.get(key, 0)])
        mats = [block_scale(k) * (tail_matrix(int(n), rng) if kind == "tail" else plan_matrix(int(n), kind, rng)) for k, (n, kind) in enumerate(zip(blk, kinds))]
        x = np.concatenate([orc.BlockIndex([M.shape[0]]).pack([M[None]]) for M in mats])
        bidx = orc.BlockIndex(blk)
        ref = orc.psd_project_svec(bidx, x)
        nrm = [max(float(np.abs(np.linalg.eigvalsh(M)).max()), 1e-300) for M in mats]          # ||M||_2 of a symmetric matrix
        for a in (x, ref):
            a.setflags(write=False)
        _INPUTS[key] = dict(blk=np.array(blk, np.int32), kinds=tuple(kinds), mats=mats, x=x, bidx=bidx, ref=ref, nrm=nrm)
    return _INPUTS[key]


def run(opts, inp):
    """-> (projection, steps per block), once per (options, input)"""
    key = (tuple(sorted(opts.items())), tuple(inp["blk"].tolist()), inp["kinds"])
    if key not in _RUNS:
        _RUNS[key] = psd_project_gpu(inp["x"], inp["blk"], opts=opts, steps=True)
    return _RUNS[key]


def check_oracle(got, inp):
    off = inp["bidx"].off
    for k, n in enumerate(inp["blk"]):
        sl = slice(int(off[k]), int(off[k + 1]))
        err, tol = np.max(np.abs(got[sl] - inp["ref"][sl])), 2e-12 * inp["nrm"][k] * np.sqrt(2)
        assert err <= tol, (k, int(n), inp["kinds"][k], err, tol)
        if inp["kinds"][k] == "psd":
            assert np.max(np.abs(got[sl] - inp["x"][sl])) <= tol          # P+ is the identity on the cone


VARIANT_CASES = [(name, tuple(blk), kind) for name, v in H.SIGN_VARIANTS.items() for blk in v["blks"] for kind in v["kinds"]]


@pytest.mark.parametrize("name,blk,kind", VARIANT_CASES, ids=["%s-%s-%s" % (n, "x".join(map(str, b)), k) for n, b, k in VARIANT_CASES])
def test_variant_vs_oracle(name, blk, kind):
    inp = inputs(blk, (kind,) * len(blk))
    got, steps = run(H.SIGN_VARIANTS[name]["opts"], inp)
    assert np.all(steps >= 1) and np.all(steps <= 64)
    check_oracle(got, inp)


@pytest.mark.parametrize("name", [n for n, v in H.SIGN_VARIANTS.items() if v["multi"]])
def test_multi_launch_variant_ends_in_both_buffers(name):
    """The final product (ROLE 3) reads the last iterate from S after an even number of steps and from T after an odd one: among the
    blocks of every multi-launch variant both must occur, or one of the two reads is untested.  (The runs are those of the test above.)"""
    v = H.SIGN_VARIANTS[name]
    counts = {}
    for blk in v["blks"]:
        for kind in v["kinds"]:
            inp = inputs(blk, (kind,) * len(blk))
            counts["x".join(map(str, blk)) + " " + kind] = run(v["opts"], inp)[1].tolist()
    print("steps %s: %s" % (name, counts))
    parities = {s & 1 for c in counts.values() for s in c}
    assert parities == {0, 1}, counts


@pytest.mark.parametrize("opts", [{}, {"psd_lg_decide": 2}], ids=["inline", "decide_kernel"])
@pytest.mark.parametrize("n", [720, 768])
def test_slots_beyond_256_carry_the_decision(n, opts):
    """276 and 300 tiles per member: the slot sum takes a second trip.  The generic families pass the oracle even when that trip is left
    out (their unresolved eigenvalues are spread over all tiles); this input keeps them in the last tile column (tail_matrix)."""
    inp = inputs((n,), ("tail",))
    got, steps = run(opts, inp)
    print("steps tail %d %s: %s" % (n, opts, steps.tolist()))
    check_oracle(got, inp)


@pytest.mark.parametrize("blk", H.SIGN_WS_CHUNKS["blks"], ids=lambda b: "x".join(map(str, b)))
def test_workspace_chunks_keep_to_their_own_state(blk):
    """psd_sign_ws_mb = 1: five blocks of 100 in chunks of 2, 2, 1 and three of 150 one by one (1 MiB does not hold one member: the chunk
    is one all the same).  Every block another family and scale, each compared with the oracle: a chunk that reads another chunk's
    schedule state, statistics or workspace shows."""
    kinds = ("moment", "randn", "graded", "lowrank", "clustered")[:len(blk)]
    inp = inputs(blk, kinds)
    got, steps = run(H.SIGN_WS_CHUNKS["opts"], inp)
    print("steps ws_mb=1 %s: %s" % (blk, steps.tolist()))
    check_oracle(got, inp)
    one_group, steps1 = run({}, inp)
    assert np.array_equal(got, one_group) and np.array_equal(steps, steps1)      # the same tile bodies on the same data


def test_no_host_polling_is_bit_identical():
    """psd_sign_sync = 0 enqueues the whole cap of the schedule and never reads the device; the launches of a finished member return at once"""
    c = H.SIGN_NO_POLL
    inp = inputs(c["blk"], ("lowrank", "moment", "clustered"))
    got, steps = run(c["opts"], inp)
    polled, steps_polled = run(c["opts_poll"], inp)
    assert np.array_equal(got, polled) and np.array_equal(steps, steps_polled)
    both = {s & 1 for s in steps.tolist()}
    print("steps no polling %s: %s" % (c["blk"], steps.tolist()))
    assert both == {0, 1}, steps
    check_oracle(got, inp)


@pytest.mark.parametrize("case", range(len(H.SIGN_STEP_CAP)), ids=["multi_launch", "one_launch"])
def test_step_cap_at_the_largest_count_changes_nothing(case):
    """psd_sign_maxsteps = the largest step count of the call: every block still finishes by its own decision, one launch before the cap"""
    opts, blk = H.SIGN_STEP_CAP[case]
    inp = inputs(blk, ("moment", "graded", "randn")[:len(blk)])
    got, steps = run(opts, inp)
    capped, steps_capped = run(dict(opts, psd_sign_maxsteps=int(steps.max())), inp)
    print("steps cap %s %s: %s" % (opts, blk, steps.tolist()))
    assert len(set(steps.tolist())) > 1                                          # a cap below some block's count would show
    assert np.array_equal(got, capped) and np.array_equal(steps, steps_capped)
    check_oracle(capped, inp)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("case", range(len(H.SIGN_NON_FINITE)), ids=["tile32", "tile64", "default_720"])
def test_multi_launch_epilogue_flags_non_finite_input(case, bad):
    """lg_pack_kernel's check (the one-launch kernel has its own in the fused epilogue, reached by test_project_sign_path_flags_non_finite_input)"""
    opts, blk = H.SIGN_NON_FINITE[case]
    inp = inputs(blk, ("randn",) * len(blk))
    member = (len(blk) - 1) if np.isinf(bad) else 0
    x = inp["x"].copy()
    x[int(inp["bidx"].off[member]) + 7] = bad                # entry (1, 3) of that member
    with pytest.raises(cuadmm_amd.CuadmmError):
        psd_project_gpu(x, inp["blk"], opts=opts)


@pytest.mark.parametrize("case", range(len(H.SIGN_ZERO_BLOCK)), ids=["tile64", "tile32", "decide_kernel"])
def test_zero_block_stays_exactly_zero(case):
    opts, blk = H.SIGN_ZERO_BLOCK[case]
    inp = inputs(blk, ("randn", "zero"))
    got, steps = run(opts, inp)
    off = inp["bidx"].off
    assert np.all(got[int(off[1]):int(off[2])] == 0.0)
    check_oracle(got, inp)


def test_one_call_with_every_kind_of_group():
    """default options: two one-launch groups sharing a launch (65; 130, 130), a multi-launch group of two members (700, 700) and the
    register kernels (40, 8) in one call"""
    c = H.SIGN_MIXED_CALL
    inp = inputs(c["blk"], ("moment", "graded", "randn", "lowrank", "clustered", "nsd", "moment"))
    got, steps = run(c["opts"], inp)
    print("steps mixed call %s: %s" % (c["blk"], steps.tolist()))
    check_oracle(got, inp)
