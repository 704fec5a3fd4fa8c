"""Certified lambda_min without a GPU ("Certified lambda_min"): the margin function against its formula, and the numpy twin
(tests/_lambda_min_twin.py) against the two properties on every matrix of the GPU test (tests/test_gpu_lambda_min.py) -- the properties
can be met before a device sees them."""
import numpy as np
import pytest

from tests._lambda_min_twin import (FAMILIES, REFINED, SIZE_CLASSES, UNREFINED, bracket, cases, check_properties, margin,
                                    reference, twin, unpack)
from tests._infeas_twin import svec


def test_margin_is_its_formula():
    rng = np.random.default_rng(0)
    for n in (1, 2, 17, 200, 1024):
        for _ in range(20):
            t, mu = rng.standard_normal() * 10.0 ** rng.integers(-5, 6), rng.random() * 10.0 ** rng.integers(-12, 3)
            want = ((n + 2) * 2.0 ** -52) * (t + n * mu)
            assert margin(n, t, mu) == want
    assert margin(3, 0.0, 0.0) == 0.0 and margin(1, 1.0, 0.0) == 3 * 2.0 ** -52
    # twice phi tr with phi = gamma_{n+1} / (1 - gamma_{n+1}), gamma_k = k u / (1 - k u), u = 2^-53, plus the rounding of the shifted diagonal
    u = 2.0 ** -53
    for n in (1, 50, 1024):
        gam = (n + 1) * u / (1 - (n + 1) * u)
        assert margin(n, 1.0, 0.0) >= 1.99 * (gam / (1 - gam) + u)


def test_unpack_inverts_svec_to_rounding():
    rng = np.random.default_rng(1)
    G = rng.standard_normal((9, 9))
    M = G + G.T
    assert np.allclose(unpack(svec(M), 9), M, rtol=4e-16, atol=0) and np.array_equal(np.diag(unpack(svec(M), 9)), np.diag(M))


@pytest.mark.parametrize("T", [6, 12])
@pytest.mark.parametrize("name", list(SIZE_CLASSES))
def test_twin_meets_the_properties(name, T):
    flags = []
    for n, fam, M, v, exact in cases(name):
        lo, hi, flag = twin(M, T)
        lam, e = reference(M) if exact is None else (exact, 0.0)
        check_properties(M, T, lo, hi, flag, lam, e, what=(n, fam))
        flags.append(flag)
        if fam == "tiny":
            assert flag == UNREFINED and lo == -bracket(M)[3]
        if fam == "neg_def" or fam == "indef_1e-3":
            assert flag == REFINED and lo < 0
    assert len(flags) == len(SIZE_CLASSES[name]) * len(FAMILIES)


def test_twin_brackets_monotonically():
    for n, fam, M, v, exact in cases("lds64"):
        lo6, lo12 = twin(M, 6)[0], twin(M, 12)[0]
        t = bracket(M)[0]
        assert lo6 <= lo12 + margin(n, max(t, 0.0), abs(lo12)), (n, fam)
