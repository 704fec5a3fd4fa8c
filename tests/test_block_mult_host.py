"""Host side of the block product (include/cuadmm_amd.h: cuadmm_block_multiply, cuadmm_op_block_mult, cuadmm_op_block_mult_plan;
csrc/block_mult.h; DESIGN.md, "Blocks times factors").  No device compute here.

The twins of tests/_block_mult_twin.py against a dense smat @ V, the wavefront task list (every 16-row panel of every PSD block in exactly
one slot, none for unconstrained blocks, slots in multiples of four with one block's panels or one-panel blocks per workgroup), the
offsets against lowrank_size, and the new entry points: present in the loaded library with their ctypes signatures, each refusing a null
argument before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import cuadmm_amd
from tests._block_mult_twin import K, LD, U, exact, host_sums, lowrank_size, pack, raw_smat, reference, unpack
from tests._infeas_twin import smat, svec

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
PANEL = 16                                      # kBmPanel (csrc/block_mult.h)


def plan(blk, rmax):
    lib = cuadmm_amd.load()
    blk = np.asarray(blk, np.int32)
    loff = np.full(blk.size + 1, -1, np.int64)
    n = lib.cuadmm_op_block_mult_plan(P(blk), blk.size, rmax, P(loff), None, 0)
    assert n >= 0 and n % 4 == 0, lib.cuadmm_last_error()
    t = np.full(2 * max(n, 1), -9, np.int32)
    assert lib.cuadmm_op_block_mult_plan(P(blk), blk.size, rmax, None, P(t), n) == n
    return loff, t[:2 * n].reshape(n, 2)


@pytest.mark.parametrize("n", [1, 2, 5, 16, 17, 40])
def test_twins_against_dense_smat(n):
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n))
    M = (G + G.T) / 2
    seg = svec(M)
    assert np.allclose(smat(seg, n), M, rtol=0, atol=1e-15)
    V = rng.standard_normal((n, min(n, 3)))
    for sign in (1.0, -1.0):
        W, A = reference(seg, n, V, sign)
        want = sign * (smat(seg, n) @ V)
        assert np.all(np.abs(W - want.astype(LD)) <= (n + 4) * LD(U) * A + 0)
    # the exact twin on small integers: the raw-slot matrix times V, the off-diagonal part scaled once per output
    seg_i = rng.integers(-3, 4, size=seg.size).astype(np.float64)
    V_i = rng.integers(-3, 4, size=V.shape).astype(np.float64)
    S = raw_smat(seg_i, n)
    offd = (S - np.diag(np.diag(S))) @ V_i
    got = exact(seg_i, n, V_i, -1.0)
    dg = np.diag(S)[:, None] * V_i
    assert np.all(np.abs(got + (K * offd + dg)) <= 4 * U * (np.abs(K * offd) + np.abs(dg)))
    Wl, A = reference(seg_i, n, V_i, -1.0)
    assert np.all(np.abs(got.astype(LD) - Wl) <= 2 * LD(U) * A)           # the constant's rounding and the final one


def test_packing_round_trip_and_host_sums():
    blk = [3, -2, 20, 1]
    rng = np.random.default_rng(0)
    Vs = [rng.standard_normal((3, 2)), np.zeros((0, 0)), rng.standard_normal((20, 5)), np.zeros((1, 0))]
    for rmax in (5, 8):
        buf, ranks = pack(blk, Vs, rmax)
        assert buf.size == lowrank_size(blk, rmax) and ranks.tolist() == [2, 77, 5, 0]
        back, pads = unpack(blk, ranks, rmax, buf)
        for a, b in zip(back, Vs):
            assert np.array_equal(a, b)
        assert all(np.all(np.isnan(p)) for p in pads) and [p.size for p in pads] == [3 * 3 - 6, 0, 20 * min(20, rmax) - 100, 1]
    pb, o = host_sums(blk, Vs, Vs)
    assert pb[:, 3].tolist() == [0, 2, 0, 0] and np.array_equal(pb[:, 0], pb[:, 2]) and pb[3, 0] == 0 and pb[1, 0] == 0
    assert np.isclose(o[0], np.sqrt(sum(np.sum(v * v) for v in Vs)), rtol=1e-14) and o[2] == 2 and o[3] == pb[2, 0] and o[4] == 3 and o[5] == 7


@pytest.mark.parametrize("rmax", [1, 4, 16, 70, 8192])
def test_plan_covers_every_panel_once(rmax):
    blk = [3, 20, -2, 70, 1, 130, -5, 300, 16, 17, 8192]
    loff, t = plan(blk, rmax)
    assert loff[0] == 0 and loff[-1] == lowrank_size(blk, rmax)
    for k in range(len(blk)):
        assert loff[k + 1] - loff[k] == lowrank_size(blk[k:k + 1], rmax)
    assert t.shape[0] % 4 == 0
    seen = {k: np.zeros(-(-n // PANEL), int) for k, n in enumerate(blk) if n > 0}
    for k, p in t:
        if k < 0:
            continue
        assert blk[k] > 0 and 0 <= p < seen[k].size, (k, p)
        seen[k][p] += 1
    assert all(np.all(c == 1) for c in seen.values())
    # a workgroup (four consecutive slots) holds panels of one block, or blocks of one panel each
    for g in t.reshape(-1, 4, 2):
        ks = [k for k, _ in g if k >= 0]
        assert len(set(ks)) == 1 or all(blk[k] <= PANEL for k in ks), g
    # the blocks of several panels come first, the largest first
    order = [k for k, p in t if k >= 0 and p == 0 and blk[k] > PANEL]
    assert [blk[k] for k in order] == sorted((n for n in blk if n > PANEL), reverse=True)


def test_plan_refuses_what_the_kernel_cannot_take():
    lib = cuadmm_amd.load()
    b = np.array([4, -2, 40], np.int32)
    assert lib.cuadmm_op_block_mult_plan(P(b), b.size, 0, None, None, 0) == -1
    assert lib.cuadmm_op_block_mult_plan(P(b), b.size, 8193, None, None, 0) == -1
    assert lib.cuadmm_op_block_mult_plan(None, 3, 4, None, None, 0) == -1
    assert lib.cuadmm_op_block_mult_plan(P(np.array([4, 0], np.int32)), 2, 4, None, None, 0) == -1
    assert lib.cuadmm_op_block_mult_plan(P(np.array([4, 8193], np.int32)), 2, 4, None, None, 0) == -1
    assert "block_mult" in lib.cuadmm_last_error().decode()
    # only unconstrained blocks: no slot, no entry
    loff, t = plan([-3, -1], 4)
    assert t.shape[0] == 0 and loff.tolist() == [0, 0, 0]


def test_symbols_signatures_and_null_refusals():
    lib = cuadmm_amd.load()
    from cuadmm_amd import _lib
    want = {"cuadmm_block_multiply": 8, "cuadmm_op_block_mult": 9, "cuadmm_op_block_mult_plan": 6}
    for name, nargs in want.items():
        assert hasattr(lib, name), name
        f = getattr(lib, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert lib.cuadmm_op_block_mult.argtypes[3] is C.c_double
    o, W, V, ranks = np.zeros(8), np.zeros(4), np.zeros(4), np.zeros(1, np.int32)
    assert lib.cuadmm_block_multiply(None, 0, P(V), P(ranks), 1, P(W), P(o), None) == -1           # CUADMM_ERR_INVALID
    assert "block_multiply" in lib.cuadmm_last_error().decode()
    fresh = cuadmm_amd.SDPSolver(verbose=False)
    assert lib.cuadmm_block_multiply(fresh._h, 0, P(V), P(ranks), 1, P(W), P(o), None) == -1          # not initialised
    blk = np.array([2], np.int32)
    for args in ((None, P(blk), 1, 1.0, P(V), P(ranks), 1, P(W)), (P(V), None, 1, 1.0, P(V), P(ranks), 1, P(W)), (P(V), P(blk), 1, 1.0, P(V), None, 1, P(W)),
                 (P(V), P(blk), 1, 1.0, P(V), P(ranks), 1, None), (P(V), P(blk), 0, 1.0, P(V), P(ranks), 1, P(W)), (P(V), P(blk), 1, 0.5, P(V), P(ranks), 1, P(W)),
                 (P(V), P(blk), 1, 1.0, P(V), P(ranks), 0, P(W)), (P(V), P(blk), 1, 1.0, P(V), P(np.array([3], np.int32)), 4, P(W)),
                 (P(V), P(blk), 1, 1.0, None, P(np.array([1], np.int32)), 4, P(W))):
        assert lib.cuadmm_op_block_mult(*args, None) == -1, args
    with pytest.raises(ValueError):
        fresh.block_multiply("y", [])
