"""cuadmm_evaluate without a device: the numpy twin (tests/_evaluate_twin.py) on points whose report is known in closed form, and the
refusals of the entry point that need no GPU (include/cuadmm_amd.h; DESIGN.md, "Evaluation of a point").
"""
import ctypes as C

import numpy as np

import cuadmm_amd
from tests._evaluate_twin import evaluate, neg_part_norm
from tests._infeas_twin import Fixture, svec
from tests._lower_bound_twin import blk_lens, make_opt_fixture

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
ERR_INVALID = -1                                          # CUADMM_ERR_INVALID (include/cuadmm_amd.h)
BLK_A, M_A = [3, 20, 70, -2, 130], 40
BLK_B, M_B = [1] * 40 + [2, 5, 8, -3, 33], 30


def test_twin_at_a_known_optimum():
    """(X*, y*, S*) of make_opt_fixture: A X* = b, A'y* + S* = C, X*, S* PSD, <X*, S*> = 0, <C, X*> = b'y*.  In exact arithmetic all six
    errors are zero; b and C of the fixture are float64 roundings of A X* and A'y* + S*, and eigh of a rank-deficient PSD block returns
    its zero eigenvalues as +-n 2^-53 ||M||: both stay below 1e-12."""
    for blk, m in ((BLK_A, M_A), (BLK_B, M_B)):
        fx = make_opt_fixture(blk, m, 1)
        t = evaluate(fx, fx.Xs, fx.ys, fx.Ss)
        errs = np.abs(t["out"][9:15])
        print(blk[-1], errs)
        assert np.all(errs <= 1e-12)
        assert abs(t["pobj"] - fx.pstar) <= 1e-12 * (1 + abs(fx.pstar))
        free = np.array(blk) < 0
        assert np.all(t["per_block"][free, 1] == 0) and np.array_equal(t["per_block"][free, 3], t["per_block"][free, 2])


def test_twin_returns_the_norm_of_the_negative_spectrum():
    rng = np.random.default_rng(3)
    blk = [4, -3, 7, 1]
    lam = {0: np.array([-2.0, -0.5, 0.0, 3.0]), 2: np.array([-1.0, -1.0, -1.0, 0.25, 0.5, 2.0, 4.0]), 3: np.array([-0.75])}
    mu = {0: np.array([1.0, 2.0, 3.0, 4.0]), 2: np.array([-3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 5.0]), 3: np.array([2.0])}
    lens = blk_lens(blk)
    off = np.concatenate([[0], np.cumsum(lens)])
    X, S = np.zeros(off[-1]), np.zeros(off[-1])
    for k, n in enumerate(blk):
        if n < 0:
            X[off[k]:off[k + 1]], S[off[k]:off[k + 1]] = [1.0, -2.0, 2.0], [0.0, 3.0, -4.0]
            continue
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        for vec, spec in ((X, lam), (S, mu)):
            M = (Q * spec[k]) @ Q.T
            vec[off[k]:off[k + 1]] = svec((M + M.T) / 2)
    m = 5
    A = rng.standard_normal((m, off[-1]))
    fx = Fixture(blk, A, rng.standard_normal(m), rng.standard_normal(off[-1]))
    y = rng.standard_normal(m)
    t = evaluate(fx, X, y, S)
    pb = t["per_block"]
    want_vX = [np.sqrt(4.25), 0.0, np.sqrt(3.0), 0.75]
    want_vS = [0.0, 5.0, 3.0, 0.0]
    assert np.allclose(pb[:, 1], want_vX, rtol=0, atol=1e-14) and np.allclose(pb[:, 3], want_vS, rtol=0, atol=1e-14)
    assert np.allclose(pb[:, 0], [np.sqrt(4 + 0.25 + 9), 3.0, np.linalg.norm(lam[2]), 0.75], rtol=1e-14)
    assert abs(pb[1, 4] - (-14.0)) <= 1e-14 and abs(pb[0, 4] - float(lam[0] @ mu[0])) <= 1e-13           # shared eigenvectors: <X_k, S_k> = lambda'mu
    assert abs(t["vX"] - np.sqrt(4.25 + 3.0 + 0.5625)) <= 1e-14 and abs(t["vS"] - np.sqrt(25.0 + 9.0)) <= 1e-14
    assert abs(neg_part_norm(svec(np.diag([-3.0, 4.0])), 2) - 3.0) <= 1e-15
    Rd = A.T @ y + S - fx.C
    assert abs(t["norm_Rd"] - np.linalg.norm(Rd)) <= 1e-13 * np.linalg.norm(Rd) and abs(t["norm_Rp"] - np.linalg.norm(A @ X - fx.b)) <= 1e-13 * t["norm_Rp"]
    den = 1 + abs(t["pobj"]) + abs(t["dobj"])
    assert t["err5"] == (t["pobj"] - t["dobj"]) / den and t["err6"] == t["XS"] / den and t["err2"] == t["vX"] / (1 + t["norm_b"])


def test_entry_point_refuses_without_a_device():
    """a created but uninitialised solver, and a null out16: CUADMM_ERR_INVALID before anything touches a device"""
    lib = cuadmm_amd.load()
    h = C.c_void_p()
    assert lib.cuadmm_create(C.byref(h)) == 0
    try:
        o = np.full(16, -7.0)
        rc = lib.cuadmm_evaluate(h, None, None, None, P(o), None)
        assert rc == ERR_INVALID
        assert "not initialised" in lib.cuadmm_last_error().decode() and np.all(o == -7.0)
        assert lib.cuadmm_evaluate(h, None, None, None, None, None) == ERR_INVALID
        assert lib.cuadmm_evaluate(None, None, None, None, P(o), None) == ERR_INVALID
        info = np.ones(4)
        assert lib.cuadmm_get_evaluate_info(h, P(info)) == 0 and np.all(info == 0)
    finally:
        lib.cuadmm_destroy(h)
