"""The one factor layout and the one factor check of the low-rank calls (csrc/factor_layout.h; DESIGN.md, "The factor layout";
include/cuadmm_amd.h: cuadmm_op_check_factors, cuadmm_op_block_outer_plan, cuadmm_op_block_mult_plan).  No device here.

The messages are written out from the format strings cuadmm_set_lowrank, cuadmm_block_multiply, cuadmm_lowrank_grad and cuadmm_lowrank_line
carried each on its own before they shared the check; nothing expected here is produced by the code under test."""
import ctypes as C

import numpy as np
import pytest

import cuadmm_amd

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
WHO = ("set_lowrank", "block_multiply", "lowrank_grad", "lowrank_line")
BLK = [3, -2, 20, 5]                            # block 2 is not the first and lies behind a free block
RMAX = 4
LOFF = [0, 9, 9, 89, 109]                       # 3 * 3, nothing, 20 * 4, 5 * 4
RANKS = [3, 77, 3, 0]                           # the free block's entry is not looked at
K, ROW, COL = 2, 7, 2                           # the entry that is spoilt: a read column of block 2
AT = LOFF[K] + COL * BLK[K] + ROW


def name_of(who):
    return "V" if who == "block_multiply" else "L"


def check(who, ranks, L, D, blk=BLK, rmax=RMAX):
    lib = cuadmm_amd.load()
    b, r = np.asarray(blk, np.int32), np.asarray(ranks, np.int32)
    rc = lib.cuadmm_op_check_factors(who.encode(), P(b), b.size, P(r), rmax, P(L), P(D))
    return rc, lib.cuadmm_last_error().decode()


def buffers():
    rng = np.random.default_rng(5)
    return rng.standard_normal(LOFF[-1]), rng.standard_normal(LOFF[-1])


@pytest.mark.parametrize("who", WHO)
def test_rank_range(who):
    L, D = buffers()
    for r, k in ((-1, 2), (min(BLK[2], RMAX) + 1, 2), (min(BLK[0], RMAX) + 1, 0)):
        ranks = list(RANKS)
        ranks[k] = r
        assert check(who, ranks, L, D) == (-1, "%s: block %d of size %d has rank %d, allowed are 0 to %d" % (who, k, BLK[k], r, min(BLK[k], RMAX)))
    # within a block the range comes before the null buffer and before the entries
    bad = L.copy()
    bad[0] = np.nan
    assert check(who, [0, 9, -1, 0], None, None)[1] == "%s: block 2 of size 20 has rank -1, allowed are 0 to 4" % who
    assert check(who, [4, 0, 0, 0], None, None)[1] == "%s: block 0 of size 3 has rank 4, allowed are 0 to 3" % who
    assert check(who, [4, 0, 0, 0], bad, D)[1] == "%s: block 0 of size 3 has rank 4, allowed are 0 to 3" % who


@pytest.mark.parametrize("who", WHO)
def test_null_buffer_with_a_positive_rank(who):
    L, D = buffers()
    # block 0 has rank 0 here: the first block that needs the buffer is named
    assert check(who, [0, 9, 3, 0], None, D) == (-1, "%s: %s is null and block 2 has rank 3" % (who, name_of(who)))
    assert check(who, RANKS, None, D) == (-1, "%s: %s is null and block 0 has rank 3" % (who, name_of(who)))
    # every rank 0: no buffer is needed
    assert check(who, [0, -3, 0, 0], None, None)[0] == 0
    if who == "lowrank_line":
        assert check(who, RANKS, L, None) == (-1, "lowrank_line: D is null and block 0 has rank 3")
        assert check(who, RANKS, None, None) == (-1, "lowrank_line: L is null and block 0 has rank 3")
    else:
        assert check(who, RANKS, L, None)[0] == 0                    # the second buffer is lowrank_line's alone


@pytest.mark.parametrize("x", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("who", WHO)
def test_entry_that_is_not_finite(who, x):
    L, D = buffers()
    bad = L.copy()
    bad[AT] = x
    if who == "lowrank_line":
        assert check(who, RANKS, bad, D) == (-1, "lowrank_line: block %d, row %d of column %d of L is not finite" % (K, ROW, COL))
        badD = D.copy()
        badD[AT] = x
        assert check(who, RANKS, L, badD) == (-1, "lowrank_line: block %d, row %d of column %d of D is not finite" % (K, ROW, COL))
        assert check(who, RANKS, bad, badD)[1] == "lowrank_line: block %d, row %d of column %d of L is not finite" % (K, ROW, COL)
        # entries are walked in order, L and D side by side: an earlier entry of D is found before a later one of L
        early = D.copy()
        early[LOFF[K] + 1] = x
        assert check(who, RANKS, bad, early)[1] == "lowrank_line: block 2, row 1 of column 0 of D is not finite"
    else:
        assert check(who, RANKS, bad, D) == (-1, "%s: block %d, row %d of column %d is not finite" % (who, K, ROW, COL))
        assert check(who, RANKS, L, bad)[0] == 0
    # the last entry that is read, and the first one
    for at, row, col in ((LOFF[K] + 3 * BLK[K] - 1, BLK[K] - 1, 2), (LOFF[K], 0, 0)):
        bad = L.copy()
        bad[at] = x
        tail = " of L" if who == "lowrank_line" else ""
        assert check(who, RANKS, bad, D)[1] == "%s: block %d, row %d of column %d%s is not finite" % (who, K, row, col, tail)


@pytest.mark.parametrize("who", WHO)
def test_what_is_not_read_is_accepted(who):
    L, D = buffers()
    for v in (L, D):
        v[LOFF[K] + 3 * BLK[K]:LOFF[K + 1]] = np.nan                # column 3 of block 2: at the rank
        v[LOFF[3]:] = np.inf                                         # block 3 has rank 0
    for free in (77, -5, 0, 2 ** 31 - 1):
        ranks = list(RANKS)
        ranks[1] = free
        assert check(who, ranks, L, D)[0] == 0, free
    assert check(who, [3, 0, 4, 0], L, D)[0] == -1                   # rank 4: the column is read now


@pytest.mark.parametrize("rmax", [1, 2, 16, 17, 8192])
@pytest.mark.parametrize("blk", [[3, 20, -2, 70, 1, 130, -5, 300], [3, 20, -2, 70, 1, 130, -5, 300, 16, 17, 8192],
                                 [1, 2, 3, 15, 16, 17, -4, 31, 32, 33, 64, 65, 130, 256, 257, 300, -1, 1100, 2000, 5], [-3, -1], [4, -2, 40]])
def test_both_plans_return_the_numpy_prefix_sum(blk, rmax):
    lib = cuadmm_amd.load()
    b = np.asarray(blk, np.int32)
    n = np.asarray(blk, np.int64)
    want = np.concatenate([[0], np.cumsum(np.where(n > 0, n * np.minimum(n, rmax), 0))])
    lo, bm = np.full(b.size + 1, -1, np.int64), np.full(b.size + 1, -1, np.int64)
    assert lib.cuadmm_op_block_outer_plan(P(b), b.size, rmax, 0, P(lo), None, 0) >= 0
    assert lib.cuadmm_op_block_mult_plan(P(b), b.size, rmax, P(bm), None, 0) >= 0
    assert np.array_equal(lo, bm) and np.array_equal(lo, want)


def test_both_plans_refuse_the_same_sizes_and_caps():
    lib = cuadmm_amd.load()
    good = np.array([4, -2, 40], np.int32)
    for b, rmax in ((np.array([4, 0], np.int32), 4), (np.array([4, 8193], np.int32), 4), (good, 0), (good, 8193)):
        assert lib.cuadmm_op_block_outer_plan(P(b), b.size, rmax, 0, None, None, 0) == -1
        assert "block_outer" in lib.cuadmm_last_error().decode()
        assert lib.cuadmm_op_block_mult_plan(P(b), b.size, rmax, None, None, 0) == -1
        assert "block_mult" in lib.cuadmm_last_error().decode()
    top = np.array([8192], np.int32)
    assert lib.cuadmm_op_block_outer_plan(P(top), 1, 8192, 0, None, None, 0) > 0 and lib.cuadmm_op_block_mult_plan(P(top), 1, 8192, None, None, 0) > 0


def test_the_hook_is_declared_like_the_others():
    lib = cuadmm_amd.load()
    from cuadmm_amd import _lib
    f = lib.cuadmm_op_check_factors
    assert f.restype is C.c_int and len(f.argtypes) == 7 == len(_lib.PROTOTYPES["cuadmm_op_check_factors"][1])
    b, r = np.array([3], np.int32), np.array([1], np.int32)
    assert f(None, P(b), 1, P(r), 1, None, None) == -1 and f(b"set_lowrank", None, 1, P(r), 1, None, None) == -1
    assert f(b"set_lowrank", P(b), 1, None, 1, None, None) == -1 and lib.cuadmm_last_error().decode() == "set_lowrank: ranks is null"
