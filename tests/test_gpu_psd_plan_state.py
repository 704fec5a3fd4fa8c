"""GPU parity of the PSD projection in the state the ENGINE keeps its plan in, at the projection's own tolerance.

tests/test_gpu_psd.py builds a fresh plan per call: no schedule hints, descriptors in build order, the null stream, one
projection.  The engine's plan lives for thousands of projections: the size classes fork to side streams and join on the caller's
non-blocking stream, every sign kernel starts its schedule from the lift count the previous projection of the block left
(sign_sched.h: "a wrong hint costs steps only"), the hints age every 16th projection, and the members of the one-wavefront classes
are re-sorted on the device while the plan is live.  Here that state is driven through the plan's test hooks
(cuadmm_psd_plan_set_hint / _reorder / _project_ordered) and every output is compared, block by block, with LAPACK
(oracle.psd_project_svec) at the bound of test_project_sign_path_spectra: max |got - ref| <= 2e-12 ||M||_2 sqrt(2).

What is asserted on is the SNAPSHOT: a copy of Xproj queued on the projection's stream right behind it, i.e. what a consumer ordered
by the stream alone sees (a class that was not joined is still NaN there); Xproj read after a device-wide synchronisation must equal it.

The spectra of every input are ones the schedule itself resolves for every hint (tests/test_sign_schedule.py:
test_schedule_resolves_the_plan_state_inputs_for_every_hint, on the CPU): a failure here is the kernels'.
"""
import numpy as np
import pytest

from oracle import cuadmm_oracle as orc
from tests.helpers import (NO_SIGN, STALE_FAMILIES, WITH_600, WITH_SIGN, PlanHandle, plan_drift_input, plan_input,
                           psd_project_gpu)

pytestmark = pytest.mark.gpu

SIGN_N_MIN = 9          # blocks from this size on run a sign kernel (they read and write hints and record steps); smaller: the register eigensolver
K_CAP = 64              # SignSched::kCap

# name -> (blocks, environment of the plan, hint_max_n)
CONFIGS = {
    "no_sign_one_wavefront": (NO_SIGN, {"CUADMM_PSD_WAVE4_MIN": "1"}, 512),     # 33 ... 64 on the one-wavefront kernels, both NP ranges
    "no_sign_one_workgroup": (NO_SIGN, {}, 512),                                # ... on the one-workgroup LDS kernels (third LDS matrix)
    "sign_launches": (WITH_SIGN, {"CUADMM_PSD_LG_CLUSTER": "0"}, 512),
    "sign_one_launch": (WITH_SIGN, {"CUADMM_PSD_LG_CLUSTER": "1"}, 512),
    "sign_600_every_group_hinted": (WITH_600, {"CUADMM_PSD_LG_CLUSTER": "1"}, 1 << 30),      # the engine's psd_hint = 2
}
PLAN_ENV = ("CUADMM_PSD_WAVE4_MIN", "CUADMM_PSD_LG_CLUSTER", "CUADMM_PSD_OVERLAP", "CUADMM_PSD_DEBUG", "CUADMM_PSD_MID", "CUADMM_PSD_N16",
            "CUADMM_PSD_N32", "CUADMM_PSD_SIGN_MIN", "CUADMM_PSD_LDS_TRIPLE", "CUADMM_PSD_LG_MERGE", "CUADMM_PSD_LG_FUSE")


class Reference:
    """LAPACK projection of x and, per block, ||M||_2"""

    def __init__(self, blocks, x):
        bidx = orc.BlockIndex(blocks)
        self.off = bidx.off
        self.ref, eigs = orc.psd_project_svec(bidx, x, return_eigs=True)
        self.nrm = np.zeros(len(blocks))
        for (n, ids, _, _, _), w in zip(bidx.groups, eigs):
            self.nrm[ids] = np.max(np.abs(w), axis=1)
        self.tol = np.repeat(2e-12 * np.maximum(self.nrm, 1e-300) * np.sqrt(2.0), np.diff(self.off))
        self.zero = np.repeat(self.nrm == 0.0, np.diff(self.off))

    def check(self, got, what):
        err = np.abs(got - self.ref)
        bad = ~(err <= self.tol)                                            # a NaN left in the output is bad
        if bad.any():
            ks = np.unique(np.searchsorted(self.off, np.flatnonzero(bad), side="right") - 1)
            worst = [(int(k), float(np.max(np.nan_to_num(err[self.off[k]:self.off[k + 1]], nan=np.inf)) / max(self.nrm[k], 1e-300))) for k in ks[:8]]
            raise AssertionError("%s: %d entries in %d blocks beyond 2e-12 ||M||_2 sqrt(2) (%d NaN); (block, max error / ||M||_2): %s" % (
                what, int(bad.sum()), ks.size, int(np.isnan(got).sum()), worst))
        assert np.all(got[self.zero] == 0.0), what + ": a zero block did not stay exactly zero"


_REFS = {}


def reference(blocks, x, key=None):
    if key is None:
        return Reference(blocks, x)
    key = (tuple(blocks), key)
    if key not in _REFS:
        _REFS[key] = Reference(blocks, x)
    return _REFS[key]


@pytest.fixture(params=list(CONFIGS))
def cfg(request, monkeypatch):
    blocks, env, hint_max_n = CONFIGS[request.param]
    for name in PLAN_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    return blocks, hint_max_n


def _signed(blocks):
    return np.array(blocks) >= SIGN_N_MIN


def _check_steps_and_hints(blocks, steps, hints_after, hints_before, what):
    s = _signed(blocks)
    assert np.all((steps[s] >= 1) & (steps[s] <= K_CAP)), (what, steps)
    assert np.all(steps[~s] == 0), (what, steps)                             # the register eigensolver records none
    if hints_after is not None:
        assert np.all((hints_after[s] >= 0) & (hints_after[s] <= K_CAP)), (what, hints_after)
        assert np.array_equal(hints_after[~s], hints_before[~s]), what       # ... and touches no hint


def test_fork_and_join_leave_every_class_in_the_snapshot(cfg):
    """No hints.  The plan on a non-blocking stream (classes forked and joined) against LAPACK, against the same plan on the null stream and
    against a fresh plan per call, bit for bit: x, -x, P(x), and an input whose side-stream blocks take ~40 steps while the caller's stream
    has next to nothing to do.  Then the four back to back into one output vector, with nothing between them but each call's wait for its own stream."""
    blocks, _ = cfg
    x0, _ = plan_input(blocks, "mixed")
    r0 = reference(blocks, x0, "mixed")
    xs = [("x", x0), ("-x", -x0), ("P(x)", r0.ref), ("sides", plan_input(blocks, "sides")[0])]
    plan = PlanHandle(blocks)
    try:
        singles = []
        for name, x in xs:
            ref = reference(blocks, x, "fork " + name)
            snap, out, steps, fails = plan.project(x, own_stream=1)
            ref.check(snap, "own stream, " + name)
            assert np.array_equal(out, snap), name
            assert fails == 0
            _check_steps_and_hints(blocks, steps, None, None, name)
            snap0, out0, steps0, fails0 = plan.project(x, own_stream=0)
            assert np.array_equal(snap0, snap) and np.array_equal(out0, snap) and np.array_equal(steps0, steps) and fails0 == 0, name
            assert np.array_equal(psd_project_gpu(x, np.array(blocks, np.int32)), snap), name
            singles.append(snap)
        snaps, fails = plan.project_back_to_back([x for _, x in xs], own_stream=1)
        assert fails == 0
        for (name, _), a, b in zip(xs, snaps, singles):
            assert np.array_equal(a, b), "back to back: " + name
    finally:
        plan.close()


def test_any_hint_costs_steps_only(cfg):
    """sign_sched.h: "A wrong hint costs steps only" -- asserted so far on the scalar host model alone.  Here on the kernels that read hints
    (one wavefront per block, one workgroup per block, the batched-GEMM groups): every hint array, the out-of-range values included (the
    kernels ignore h <= 0, decide() clamps lift0 into [1, kCap]), leaves the projection within the bound, no failure, steps in [1, 64]
    and hints in [0, 64].  The hints a projection leaves, used as the next input, give the same bits, steps and hints on every rerun, and
    iterating h -> h' four times more keeps the bound and the ranges.  That h' = h is NOT asserted: a run whose first lift phase was too
    short adds bursts, and its lift count, taken up front the next time, is another schedule.  Seen on the MI355X: from zero hints 16 of 60 blocks (no sign path)
    to 20 of 68 (with the n = 600 block) take another number of steps on the next run and 8 to 12 still do four runs later; from hints
    at the cap none does (the counts are printed)."""
    blocks, hint_max_n = cfg
    x, _ = plan_input(blocks, "mixed")
    ref = reference(blocks, x, "mixed")
    rng = np.random.default_rng(5)
    nb = len(blocks)
    arrays = [("zeros", np.zeros(nb, np.int32)), ("ones", np.ones(nb, np.int32)), ("cap", np.full(nb, K_CAP, np.int32)),
              ("random", rng.integers(0, K_CAP + 1, nb).astype(np.int32)),
              ("out of range", np.resize(np.array([-5, 65, 1000, 2 ** 31 - 1], np.int32), nb))]
    for name, h0 in arrays:
        plan = PlanHandle(blocks)                                            # a plan per array: none of its projections is aged
        try:
            plan.set_hint(h0, hint_max_n)
            snap, out, steps, fails = plan.project(x, own_stream=1)
            ref.check(snap, name)
            assert np.array_equal(out, snap) and fails == 0, name
            h1 = plan.get_hint()
            _check_steps_and_hints(blocks, steps, h1, h0, name)
            runs = []
            for _ in range(2):
                plan.set_hint(h1, hint_max_n)
                snap2, out2, steps2, fails2 = plan.project(x, own_stream=1)
                runs.append((snap2, steps2, plan.get_hint()))
                assert np.array_equal(out2, snap2) and fails2 == 0, name
            ref.check(runs[0][0], name + ", its own hints")
            _check_steps_and_hints(blocks, runs[0][1], runs[0][2], h1, name + ", its own hints")
            assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1])), name
            changed = [int(np.sum(runs[0][1] != steps))]
            h, prev_steps = runs[0][2], runs[0][1]
            for it in range(4):                                              # the plan keeps the hints it wrote: h -> h' as in the engine
                snap3, out3, steps3, fails3 = plan.project(x, own_stream=1)
                ref.check(snap3, "%s, iteration %d of its hints" % (name, it))
                assert np.array_equal(out3, snap3) and fails3 == 0, (name, it)
                h_next = plan.get_hint()
                _check_steps_and_hints(blocks, steps3, h_next, h, (name, it))
                changed.append(int(np.sum(steps3 != prev_steps)))
                h, prev_steps = h_next, steps3
            print("hints %-12s: blocks whose step count changed from one run to the next: %s" % (name, changed))
            assert plan.hinted_projections < 16
        finally:
            plan.close()


def test_stale_hints_across_a_change_of_spectrum(cfg):
    """Every block projects family A, then -- with the hints that left -- family B, for every ordered pair: ~30 lifts learned on a moment
    matrix applied to a PSD or a zero block and the reverse are the sharpest.  (The plan ages the hints on every 16th projection on top.)"""
    blocks, hint_max_n = cfg
    plan = PlanHandle(blocks)
    try:
        left = {}
        for fam in STALE_FAMILIES:
            x, _ = plan_input(blocks, fam)
            plan.set_hint(np.zeros(len(blocks), np.int32), hint_max_n)
            snap, out, steps, fails = plan.project(x, own_stream=1)
            reference(blocks, x, fam).check(snap, fam)
            assert np.array_equal(out, snap) and fails == 0, fam
            left[fam] = plan.get_hint()
        for a in STALE_FAMILIES:
            for b in STALE_FAMILIES:
                x, _ = plan_input(blocks, b)
                plan.set_hint(left[a], hint_max_n)
                snap, out, steps, fails = plan.project(x, own_stream=1)
                reference(blocks, x, b).check(snap, "%s after %s" % (b, a))
                assert np.array_equal(out, snap) and fails == 0, (a, b)
                h = plan.get_hint()
                s = _signed(blocks)
                assert np.all((steps[s] >= 1) & (steps[s] <= K_CAP)) and np.all((h[s] >= 0) & (h[s] <= K_CAP)), (a, b)
    finally:
        plan.close()


def _aged(h):
    return np.where(h > 1, h - 1, h)          # hint_decay_kernel


def test_hints_age_every_sixteenth_projection(cfg):
    """33 projections of one input with hints on: within the bound every time, hints in [0, 64]; the 16th and the 32nd start from the hints
    of the one before less one lift step (hint_decay_kernel) -- a second plan given exactly those hints leaves the same bits, steps and hints."""
    blocks, hint_max_n = cfg
    x, _ = plan_input(blocks, "mixed")
    ref = reference(blocks, x, "mixed")
    plan, twin = PlanHandle(blocks), PlanHandle(blocks)
    try:
        plan.set_hint(np.zeros(len(blocks), np.int32), hint_max_n)
        before = np.zeros(len(blocks), np.int32)
        for k in range(1, 34):
            snap, out, steps, fails = plan.project(x, own_stream=1)
            ref.check(snap, "projection %d" % k)
            assert np.array_equal(out, snap) and fails == 0, k
            h = plan.get_hint()
            s = _signed(blocks)
            assert np.all((h[s] >= 0) & (h[s] <= K_CAP)) and np.all(h[~s] == 0), (k, h)
            if k % 16 == 0:
                twin.set_hint(_aged(before), hint_max_n)
                snap_t, _, steps_t, _ = twin.project(x, own_stream=1)
                assert np.array_equal(snap_t, snap) and np.array_equal(steps_t, steps) and np.array_equal(twin.get_hint(), h), k
            before = h
        assert plan.hinted_projections == 33 and twin.hinted_projections == 2
    finally:
        plan.close(); twin.close()


def test_reordering_permutes_work_not_results(cfg):
    """reorder_by_steps / _async re-sort the members' descriptors of the one-wavefront classes on the device, range by range: the
    projection behind it must not differ by one bit (every block has its own scale: a descriptor in the wrong range or at the wrong
    offset cannot pass), whatever the step counts say -- equal, increasing, decreasing, beyond kCap + 1, negative.  With hints on, the
    hints follow the block, not the slot."""
    blocks, hint_max_n = cfg
    nb = len(blocks)
    x, _ = plan_input(blocks, "mixed")
    ref = reference(blocks, x, "mixed")
    rng = np.random.default_rng(9)
    plan = PlanHandle(blocks)
    try:
        snap0, out0, steps0, fails = plan.project(x, own_stream=1)
        ref.check(snap0, "build order")
        assert np.array_equal(out0, snap0) and fails == 0
        some_negative = rng.integers(-40, 41, nb).astype(np.int32)
        assert (some_negative < 0).any()
        orders = [("recorded", steps0), ("equal", np.full(nb, 7, np.int32)), ("increasing", np.arange(nb, dtype=np.int32) % 65),
                  ("decreasing", (nb - np.arange(nb, dtype=np.int32)) % 65), ("random beyond the cap", rng.integers(0, 71, nb).astype(np.int32)),
                  ("some negative", some_negative)]
        for name, steps in orders:
            for async_ in (0, 1):
                plan.reorder(steps, async_=async_, own_stream=1)
                snap, out, st, fails = plan.project(x, own_stream=1)
                assert np.array_equal(snap, snap0), (name, async_)
                assert np.array_equal(out, snap) and np.array_equal(st, steps0) and fails == 0, (name, async_)
    finally:
        plan.close()
    plain, sorted_ = PlanHandle(blocks), PlanHandle(blocks)
    try:
        for p in (plain, sorted_):
            p.set_hint(np.zeros(nb, np.int32), hint_max_n)
        first = plain.project(x, own_stream=1)
        first_s = sorted_.project(x, own_stream=1)
        assert np.array_equal(first[0], first_s[0]) and np.array_equal(plain.get_hint(), sorted_.get_hint())
        sorted_.reorder(rng.integers(0, 71, nb).astype(np.int32), async_=1, own_stream=1)
        second = plain.project(x, own_stream=1)
        second_s = sorted_.project(x, own_stream=1)
        ref.check(second_s[0], "hints on, re-sorted")
        assert np.array_equal(second[0], second_s[0]) and np.array_equal(second[2], second_s[2])
        assert np.array_equal(plain.get_hint(), sorted_.get_hint())
    finally:
        plain.close(); sorted_.close()


def test_everything_together_as_the_engine_runs_it(monkeypatch):
    """A non-blocking stream, hints on, small classes beside the one-launch sign path: 20 projections of a slowly drifting input with a
    jump to -x_0 at k = 10 (every hint stale at once), re-sorted by the recorded steps at k = 3 without draining the stream."""
    blocks, env, hint_max_n = CONFIGS["sign_one_launch"]
    for name in PLAN_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    plan = PlanHandle(blocks)
    try:
        plan.set_hint(np.zeros(len(blocks), np.int32), hint_max_n)
        for k in range(20):
            x = plan_drift_input(blocks, k)
            snap, out, steps, fails = plan.project(x, own_stream=1)
            reference(blocks, x).check(snap, "k = %d" % k)
            assert np.array_equal(out, snap) and fails == 0, k
            h = plan.get_hint()
            _check_steps_and_hints(blocks, steps, h, np.zeros(len(blocks), np.int32), "k = %d" % k)
            if k == 3:
                plan.reorder(steps, async_=1, own_stream=1)
    finally:
        plan.close()
