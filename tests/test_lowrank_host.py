"""Host side of the per-block pivoted Cholesky (include/cuadmm_amd.h: cuadmm_lowrank, cuadmm_lowrank_size, cuadmm_op_block_lowrank;
DESIGN.md, "Low-rank factors").  No device compute here.

The numpy twin (tests/_lowrank_twin.py) alone meets the four statements of the factor on every case of every size the GPU test runs, and
reports the rank r0 on the lowrank_* families: the tolerances of check_properties, none of them measured, are reachable by a correct
implementation.  Then the new entry points: present in the loaded library, and each refuses a null handle or vector before it touches a
device."""
import ctypes as C

import numpy as np
import pytest

import cuadmm_amd
from tests._lowrank_twin import (CAPPED, COMPLETE, NOT_FACTORED, SIZES, TOL, cases, check_properties, lowrank_size, pack, split, twin, unpack)

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n", list(SIZES))
def test_twin_meets_the_four_statements(n):
    rmax = SIZES[n][0]
    for c in cases(n):
        M, fam = c["M"], c["family"]
        rank, resid, dneg, t, flag, L, piv = twin(M, TOL, rmax)
        what = (n, fam)
        if fam == "nan":
            assert (rank, flag) == (0, NOT_FACTORED) and np.isnan(resid) and np.all(L == 0.0) and np.all(piv == -1), what
            continue
        check_properties(M, TOL, rmax, rank, resid, dneg, flag, L, piv, psd=c["psd"], what=what)
        assert abs(t - np.trace(M)) <= n * 2.0 ** -53 * np.abs(np.diag(M)).sum(), what
        if c["r0"] is not None:
            assert rank == min(c["r0"], rmax) and flag == (CAPPED if c["r0"] > rmax else COMPLETE), (what, rank, flag)
        if fam == "identity":
            assert np.array_equal(piv, np.arange(n)), what                     # ties: the smallest index
        if fam == "zero":
            assert (rank, resid, dneg, flag) == (0, 0.0, 0.0, COMPLETE), what
        if fam == "indef":
            assert dneg <= -0.25 and n // 2 not in piv[:rank].tolist(), (what, dneg)


@pytest.mark.parametrize("n", [n for n in SIZES if SIZES[n][1] is None and n >= 2])
def test_twin_scales_exactly_with_powers_of_four(n):
    rmax = SIZES[n][0]
    by = {c["family"]: c for c in cases(n)}
    base = twin(by["lowrank_2"]["M"], TOL, rmax)
    for fam, e in (("scaled_down", -200), ("scaled_up", 200)):
        got = twin(by[fam]["M"], TOL, rmax)
        assert got[0] == base[0] == 2 and got[4] == base[4] and np.array_equal(got[6], base[6]), (n, fam)
        assert np.array_equal(got[5], base[5] * 2.0 ** e), (n, fam)


def test_pack_and_split_round_trip():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((5, 5))
    M = unpack(pack(A + A.T), 5)
    assert np.array_equal(M, M.T) and np.allclose(M, A + A.T, rtol=1e-15, atol=0)
    blk, rmax = [3, -2, 5], 4
    assert lowrank_size(blk, rmax) == 3 * 3 + 5 * 4
    per = np.array([[1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 2, 9], [2, 0, 0, 0, 0, 9]], float).ravel()
    L, piv = np.arange(29.0), np.arange(29)
    parts = split(blk, rmax, per, L, piv)
    assert parts[0][5].shape == (3, 3) and parts[1][5].shape == (0, 0) and parts[2][5].shape == (5, 4)
    assert parts[2][5][1, 2] == 9 + 2 * 5 + 1 and list(parts[2][6]) == [9, 10, 11, 12]


def test_the_entry_points_exist_and_refuse_null_arguments():
    lib = cuadmm_amd.load()
    raw = C.CDLL(cuadmm_amd.LIB_PATH)
    for name in ("cuadmm_lowrank", "cuadmm_lowrank_size", "cuadmm_op_block_lowrank"):
        getattr(raw, name)
    o, pb, count = np.zeros(8), np.zeros(6), C.c_longlong(-7)
    blk = np.array([3], np.int32)
    assert lib.cuadmm_lowrank(None, 0, 1e-8, 4, P(o), None, None, None) == -1            # CUADMM_ERR_INVALID
    assert "lowrank" in lib.cuadmm_last_error().decode()
    assert lib.cuadmm_op_block_lowrank(None, P(blk), 1, 1e-8, 4, P(pb), None, None, None) == -1
    assert lib.cuadmm_lowrank_size(None, 4, C.byref(count)) == -1 and count.value == -7
    fresh = cuadmm_amd.SDPSolver(verbose=False)                                           # created, not initialised: no blocks to count
    assert lib.cuadmm_lowrank_size(fresh._h, 4, C.byref(count)) == -1
    assert lib.cuadmm_lowrank(fresh._h, 0, 1e-8, 4, P(o), None, None, None) == -1
