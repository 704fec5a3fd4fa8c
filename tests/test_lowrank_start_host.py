"""Host side of the start from low-rank factors (include/cuadmm_amd.h: cuadmm_set_lowrank, cuadmm_op_block_outer,
cuadmm_op_block_outer_plan; csrc/lowrank_apply.h; DESIGN.md, "Starting from low-rank factors").  No device compute here.

The offsets of the factor buffer against lowrank_size and split of tests/_lowrank_twin.py, the wavefront task list (every tile of every
PSD block exactly once, the three size classes, the split size lowered), the Python packing of a list of (n_k, r_k) arrays into that
layout, and the new entry points: present in the loaded library, each refusing a null argument before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd.solver import pack_lowrank
from tests._lowrank_twin import lowrank_size, split

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
WAVE_MAX, SPLIT_FROM, RUN = 32, 257, 32          # kLoWaveMax, kLoSplitFrom, kLoRunTiles (csrc/lowrank_apply.h)


def tiles(n):
    nt = -(-n // 16)
    return nt * (nt + 1) // 2


def plan(blk, rmax, split_from=0):
    lib = cuadmm_amd.load()
    blk = np.asarray(blk, np.int32)
    loff = np.full(blk.size + 1, -1, np.int64)
    n = lib.cuadmm_op_block_outer_plan(P(blk), blk.size, rmax, split_from, P(loff), None, 0)
    assert n >= 0 and n % 4 == 0, lib.cuadmm_last_error()
    t = np.full(4 * max(n, 1), -9, np.int32)
    assert lib.cuadmm_op_block_outer_plan(P(blk), blk.size, rmax, split_from, None, P(t), n) == n
    return loff, t[:4 * n].reshape(n, 4)


@pytest.mark.parametrize("rmax", [1, 4, 16, 70, 8192])
def test_offsets_are_those_of_the_lowrank_layout(rmax):
    blk = [3, 20, -2, 70, 1, 130, -5, 300]
    loff, _ = plan(blk, rmax)
    assert loff[0] == 0 and loff[-1] == lowrank_size(blk, rmax)
    for k in range(len(blk)):
        assert loff[k + 1] - loff[k] == lowrank_size(blk[k:k + 1], rmax)
    # split() of the twin reads block k's factor at per_block[k, 5]: with the plan's offsets it finds what the Python packing put there
    rng = np.random.default_rng(rmax)
    Ls = [rng.standard_normal((max(n, 0), min(max(n, 0), rmax))) for n in blk]
    L, ranks, rm = pack_lowrank(blk, Ls)
    assert rm == max(1, min(rmax, 300)) and L.size == loff2(blk, rm)[-1]
    per = np.zeros((len(blk), 6))
    per[:, 5] = loff2(blk, rm)[:-1]
    for k, part in enumerate(split(blk, rm, per.ravel(), L, np.zeros(L.size, np.int32))):
        if blk[k] > 0:
            assert np.array_equal(part[5][:, :ranks[k]], Ls[k])


def loff2(blk, rmax):
    return plan(blk, rmax)[0]


def _check_cover(blk, t, split_from):
    seen = {k: np.zeros(tiles(n), int) for k, n in enumerate(blk) if n > 0}
    for q, (k, t0, t1, step) in enumerate(t):
        if k < 0:
            continue
        assert blk[k] > 0 and step in (1, 4) and 0 <= t0 and t1 <= tiles(blk[k])
        seen[k][t0:t1:step] += 1
    for k, c in seen.items():
        assert np.all(c == 1), (k, blk[k])                                   # every tile of every PSD block, once
    for k, n in enumerate(blk):
        slots = np.flatnonzero(t[:, 0] == k)
        if n <= 0:
            assert slots.size == 0
        elif n <= WAVE_MAX:
            assert slots.size == 1 and tuple(t[slots[0], 1:]) == (0, tiles(n), 1)
        elif n < split_from:                                                  # one workgroup: four consecutive slots, aligned
            assert slots.size == 4 and slots[0] % 4 == 0 and np.array_equal(slots, slots[0] + np.arange(4))
            assert t[slots, 1].tolist() == [0, 1, 2, 3] and np.all(t[slots, 2] == tiles(n)) and np.all(t[slots, 3] == 4)
        else:                                                                 # runs of RUN tiles, one workgroup each
            assert slots.size == 4 * -(-tiles(n) // RUN) and np.all(slots.reshape(-1, 4)[:, 0] % 4 == 0)
            for g in slots.reshape(-1, 4):
                assert np.array_equal(g, g[0] + np.arange(4)) and np.array_equal(t[g, 1], t[g[0], 1] + np.arange(4))
                assert t[g[0], 1] % RUN == 0 and np.all(t[g, 2] == min(t[g[0], 1] + RUN, tiles(n)))


def test_task_list_covers_every_tile_once_in_three_size_classes():
    blk = [1, 2, 3, 15, 16, 17, -4, 31, 32, 33, 64, 65, 130, 256, 257, 300, -1, 1100, 2000, 5]
    _, t = plan(blk, 16)
    _check_cover(blk, t, SPLIT_FROM)
    # one block of 2000 is dealt to about as many workgroups as the device has compute units
    assert np.sum(t[:, 0] == blk.index(2000)) // 4 == -(-tiles(2000) // RUN) == 247
    # the list does not depend on rmax, the split size can be lowered down to 33
    assert np.array_equal(plan(blk, 1)[1], t)
    _, t2 = plan(blk, 16, split_from=65)
    _check_cover(blk, t2, 65)
    assert np.sum(t2[:, 0] == blk.index(130)) == 4 * -(-tiles(130) // RUN) > 4
    lib = cuadmm_amd.load()
    b = np.asarray(blk, np.int32)
    assert lib.cuadmm_op_block_outer_plan(P(b), b.size, 16, 32, None, None, 0) == -1
    assert lib.cuadmm_op_block_outer_plan(P(b), b.size, 0, 0, None, None, 0) == -1
    assert lib.cuadmm_op_block_outer_plan(P(np.array([4, 0], np.int32)), 2, 4, 0, None, None, 0) == -1
    # only unconstrained blocks: nothing to do
    assert plan([-3, -1], 4)[1].shape == (0, 4)


def test_python_packing_of_a_list_of_factors():
    blk = [3, -2, 5, 4]
    A = [np.arange(6.0).reshape(3, 2) + 1, np.zeros((7, 7)), np.arange(15.0).reshape(5, 3) + 10, np.zeros((4, 0))]
    L, ranks, rmax = pack_lowrank(blk, A)
    assert rmax == 3 and ranks.tolist() == [2, 0, 3, 0] and ranks.dtype == np.int32
    assert L.size == lowrank_size(blk, 3) == 9 + 15 + 12
    want = np.zeros(36)
    for k, o in ((0, 0), (2, 9)):
        for c in range(A[k].shape[1]):
            for i in range(A[k].shape[0]):
                want[o + c * A[k].shape[0] + i] = A[k][i, c]
    assert np.array_equal(L, want)
    # every rank 0: rmax = 1, a buffer of the layout's size; what lowrank() returns for an unconstrained block, (0, 0), is accepted
    L0, r0, m0 = pack_lowrank([3, -2], [np.zeros((3, 0)), np.zeros((0, 0))])
    assert m0 == 1 and r0.tolist() == [0, 0] and L0.size == 3 and not L0.any()
    for bad in ([np.zeros((4, 2)), None, A[2], A[3]], [np.zeros((3, 4)), None, A[2], A[3]], [np.zeros(3), None, A[2], A[3]], A[:3]):
        with pytest.raises(ValueError):
            pack_lowrank(blk, bad)


def test_the_entry_points_exist_and_refuse_null_arguments():
    lib = cuadmm_amd.load()
    raw = C.CDLL(cuadmm_amd.LIB_PATH)
    for name in ("cuadmm_set_lowrank", "cuadmm_op_block_outer", "cuadmm_op_block_outer_plan"):
        getattr(raw, name)
    ranks, blk, L, o = np.array([1], np.int32), np.array([3], np.int32), np.ones(3), np.zeros(4)
    assert lib.cuadmm_set_lowrank(None, 0, P(L), P(ranks), 1, 0.0, P(o)) == -1            # CUADMM_ERR_INVALID
    assert "set_lowrank" in lib.cuadmm_last_error().decode()
    fresh = cuadmm_amd.SDPSolver(verbose=False)                                           # created, not initialised
    assert lib.cuadmm_set_lowrank(fresh._h, 0, P(L), P(ranks), 1, 0.0, P(o)) == -1
    for args in ((P(L), None, P(blk), 1, 1, 1), (P(L), P(ranks), None, 1, 1, 1), (P(L), P(ranks), P(blk), 1, 1, None), (P(L), P(ranks), P(blk), 1, 0, 1),
                 (None, P(ranks), P(blk), 1, 1, 1), (P(L), P(np.array([2], np.int32)), P(blk), 1, 1, 1), (P(L), P(np.array([-1], np.int32)), P(blk), 1, 1, 1)):
        assert lib.cuadmm_op_block_outer(*args, None) == -1, args
    assert not o.any()
