"""GPU parity: fused PSD projection and the eigensolver vs the oracle (LAPACK dsyevd path).

Tolerances: projection <= 1e-12 * max(1,||X_blk||_F) per entry; eigenvalues
<= 1e-12 * ||A||_2; svec index layout bit-exact (checked through the round-trip of PSD inputs).
"""
import numpy as np
import pytest

from oracle import cuadmm_oracle as orc
from tests.helpers import batch_eig_gpu, psd_project_gpu

pytestmark = pytest.mark.gpu


def _rand_svec(blk, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    L = int(orc.svec_block_offsets(blk)[-1])
    return rng.standard_normal(L) * scale


@pytest.mark.parametrize("blk", [
    [1], [2], [3], [4], [5], [8], [9], [16], [17], [31], [32],
    [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32],
    [32] * 7, [6] * 37 + [4], [1] * 100 + [2] * 33,
])
def test_project_small_blocks(blk):
    blk = np.array(blk, dtype=np.int32)
    x = _rand_svec(blk, 11)
    got = psd_project_gpu(x, blk)
    ref = orc.psd_project_svec(orc.BlockIndex(blk), x)
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(x)) * 32)


@pytest.mark.parametrize("blk", [[33], [55], [64], [65], [91], [120], [128], [130], [33, 40, 64, 100]])
def test_project_mid_blocks(blk):
    blk = np.array(blk, dtype=np.int32)
    x = _rand_svec(blk, 12)
    got = psd_project_gpu(x, blk)
    ref = orc.psd_project_svec(orc.BlockIndex(blk), x)
    assert np.max(np.abs(got - ref)) <= 2e-12 * max(1.0, np.max(np.abs(x)) * blk.max())


@pytest.mark.parametrize("n", [150, 300])
def test_project_large_block_hbm_path(n):
    blk = np.array([n], dtype=np.int32)
    x = _rand_svec(blk, 13)
    got = psd_project_gpu(x, blk)
    ref = orc.psd_project_svec(orc.BlockIndex(blk), x)
    assert np.max(np.abs(got - ref)) <= 5e-12 * n


def test_project_mixed_planarhand_sizes():
    blk = np.array([7] * 5 + [10] * 12 + [11] * 26 + [13] * 14 + [15] * 51 + [28] * 3 + [55] * 2 + [66] * 3 + [91] * 3 + [120] * 3,
                   dtype=np.int32)
    rng = np.random.default_rng(3)
    blk = blk[rng.permutation(blk.size)]
    x = _rand_svec(blk, 14)
    got = psd_project_gpu(x, blk)
    ref = orc.psd_project_svec(orc.BlockIndex(blk), x)
    assert np.max(np.abs(got - ref)) <= 2e-12 * 120


def test_project_properties_full_size():
    """BASELINE config 2 size (10 000 blocks of 32): idempotence, PSD inputs fixed, NSD inputs -> 0."""
    blk = np.full(10000, 32, dtype=np.int32)
    bidx = orc.BlockIndex(blk)
    x = _rand_svec(blk, 15)
    p1 = psd_project_gpu(x, blk)
    p2 = psd_project_gpu(p1, blk)
    scale = np.max(np.abs(x)) * 32
    assert np.max(np.abs(p2 - p1)) <= 1e-12 * scale                     # idempotent
    # Moreau: x = P+(x) - P+(-x)
    pm = psd_project_gpu(-x, blk)
    assert np.max(np.abs((p1 - pm) - x)) <= 1e-12 * scale
    # <P+(x), P+(-x)> = 0 per block (complementarity), checked in aggregate
    assert abs(np.dot(p1, pm)) <= 1e-10 * np.dot(x, x)
    # spot-check 64 random blocks against the oracle
    sel = np.random.default_rng(0).choice(10000, 64, replace=False)
    for k in sel:
        sl = slice(int(bidx.off[k]), int(bidx.off[k + 1]))
        ref = orc.psd_project_svec(orc.BlockIndex([32]), x[sl])
        assert np.max(np.abs(p1[sl] - ref)) <= 1e-12 * scale


def test_project_edge_inputs():
    blk = np.array([32, 32, 16, 5, 32, 1, 1], dtype=np.int32)
    bidx = orc.BlockIndex(blk)
    L = int(bidx.off[-1])
    x = np.zeros(L)
    rng = np.random.default_rng(5)
    # block 0: zero matrix; block 1: identity (already diagonal); block 2: diagonal with mixed signs;
    # block 3: rank one; block 4: repeated eigenvalues; blocks 5,6: scalars +/-.
    mats = [np.zeros((32, 32)), np.eye(32), np.diag(rng.standard_normal(16))]
    v = rng.standard_normal(5); mats.append(np.outer(v, v))
    Q, _ = np.linalg.qr(rng.standard_normal((32, 32)))
    lam = np.repeat([-2.0, 0.0, 3.0, 3.0], 8)
    mats.append((Q * lam) @ Q.T)
    mats += [np.array([[2.5]]), np.array([[-1.5]])]
    for k, M in enumerate(mats):
        x[int(bidx.off[k]):int(bidx.off[k + 1])] = orc.BlockIndex([M.shape[0]]).pack([M[None]])
    got = psd_project_gpu(x, blk)
    ref = orc.psd_project_svec(bidx, x)
    assert np.max(np.abs(got - ref)) <= 1e-12 * 10
    assert np.all(got[:int(bidx.off[1])] == 0.0)                         # zero block stays exactly zero
    assert got[-1] == 0.0 and got[-2] == 2.5


@pytest.mark.parametrize("n", [5, 16, 28, 32, 55, 91, 120])
def test_project_rank_deficient_and_graded(n):
    """Moment-matrix-like inputs: rank one (one O(1) eigenvalue, the rest at roundoff level), rank two shifted
    slightly negative, and a spectrum graded over 20 decades -- the cases where a purely local QL
    deflation test stagnates (seen on PlanarHand_N=1 block 0, n=91, iteration 2)."""
    rng = np.random.default_rng(n)
    mats = []
    v = rng.standard_normal(n); mats.append(np.outer(v, v))
    u = rng.standard_normal((n, 2)); mats.append(u @ u.T - 1e-9 * np.eye(n))
    Q, _ = np.linalg.qr(rng.standard_normal((n, n))); mats.append((Q * np.logspace(-18, 2, n)) @ Q.T)
    mats.append(-mats[0])
    blk = np.full(len(mats), n, dtype=np.int32)
    bidx = orc.BlockIndex(blk)
    x = bidx.pack([np.stack(mats)])
    got = psd_project_gpu(x, blk)
    ref = orc.psd_project_svec(bidx, x)
    assert np.max(np.abs(got - ref)) <= 1e-13 * n * max(1.0, np.max(np.abs(x)))


@pytest.mark.parametrize("n,count", [(2, 5), (3, 4), (4, 3), (6, 100), (10, 33), (16, 17), (32, 64), (45, 5), (105, 2), (200, 1)])
def test_batch_eig_vs_lapack(n, count):
    rng = np.random.default_rng(n * 1000 + count)
    A = rng.standard_normal((count, n, n))
    A = (A + np.swapaxes(A, 1, 2)) / 2
    W, V, info = batch_eig_gpu(A)
    assert np.all(info == 0)
    w_ref = np.linalg.eigvalsh(A)
    nrm = np.max(np.abs(w_ref))
    assert np.max(np.abs(W - w_ref)) <= 1e-12 * nrm * max(1, n / 8)
    assert np.all(np.diff(W, axis=1) >= 0)                               # ascending (sort_eig=1, cusolver.h:112-123)
    rec = np.einsum("bik,bk,bjk->bij", V, W, V)
    assert np.max(np.abs(rec - A)) <= 5e-13 * nrm * n
    orth = np.einsum("bki,bkj->bij", V, V) - np.eye(n)
    assert np.max(np.abs(orth)) <= 5e-13 * n


def _eig_family(n, kind, rng):
    if kind == "randn":
        G = rng.standard_normal((n, n)); return (G + G.T) / 2
    if kind == "rank1":
        v = rng.standard_normal(n); return np.outer(v, v)
    if kind == "lowrank":                 # late-ADMM iterate: rank 5 plus indefinite noise at 1e-7
        U = rng.standard_normal((n, 5)); G = rng.standard_normal((n, n)); return U @ U.T + 1e-7 * (G + G.T)
    if kind == "identity":
        return np.eye(n)
    if kind == "zero":
        return np.zeros((n, n))
    if kind == "diag":
        return np.diag(rng.standard_normal(n))
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    if kind == "graded":                  # both signs over 14 decades
        w = np.logspace(-14, 0, n) * np.where(np.arange(n) % 2, 1.0, -1.0)
    elif kind == "clustered":             # five eigenvalues, each n / 5 times (two of them 1e-9 apart)
        w = np.repeat(np.array([-2.0, -1e-3, 0.0, 1.0, 1.0 + 1e-9]), (n + 4) // 5)[:n]
    else:                                 # "tight": pairs 1e-13 apart
        w = np.repeat(np.linspace(-1, 1, (n + 1) // 2), 2)[:n] + np.tile([0.0, 1e-13], (n + 1) // 2)[:n]
    M = (Q * w) @ Q.T
    return (M + M.T) / 2


def _check_eig(A, W, V, info):
    n = A.shape[0]
    assert info == 0
    w = np.linalg.eigvalsh(A)
    nrm = np.abs(w).max() + 1e-290                                      # the zero matrix: the bisection answers +-pivmin ~ 1e-308
    assert np.max(np.abs(W - w)) <= 1e-12 * nrm                         # eigenvalues <= 1e-12 ||A||_2
    assert np.all(np.diff(W) >= 0)                                      # ascending (cusolver.h:76-95)
    assert np.max(np.abs((V * W[None, :]) @ V.T - A)) <= 1e-12 * nrm    # reconstruction
    assert np.max(np.abs(V.T @ V - np.eye(n))) <= 1e-12                 # orthogonality


@pytest.mark.parametrize("kind", ["randn", "rank1", "lowrank", "identity", "zero", "diag", "graded", "clustered", "tight"])
@pytest.mark.parametrize("n", [129, 257, 500])
def test_batch_eig_whole_chip_path_spectra(n, kind):
    """single_eig_cusolver contract (include/cuadmm/cusolver.h:76-95: Xsyevd, W ascending, V in place; call loop
    src/solver.cu:540-564) for n >= 129: tridiagonalisation over the chip, bisection, inverse iteration, Cholesky-QR
    (csrc/eig_large.hip), on spectra that stress each phase: multiple / tightly clustered eigenvalues (the orthonormalisation),
    rank-deficient and graded (the bisection's absolute accuracy), diagonal / identity / zero (no reflectors at all)."""
    A = _eig_family(n, kind, np.random.default_rng(n))
    W, V, info = batch_eig_gpu(A[None])
    _check_eig(A, W[0], V[0], int(info[0]))


@pytest.mark.parametrize("n", [1024, 2000])
def test_batch_eig_large_block_at_the_baseline_size_under_a_second(n):
    """BASELINE configs[2] is one block of n ~ 2000.  Round 2 ran one workgroup (3.2 s at n = 1024, 76 s at n = 2000, fenced
    above 1024); the whole-chip path needs ~0.1 s including the 32 MB copies of this test."""
    import time
    rng = np.random.default_rng(77)
    G = rng.standard_normal((n, n))
    A = (G + G.T) / 2
    batch_eig_gpu(A[None])                                              # first call: code objects, allocator
    t0 = time.time()
    W, V, info = batch_eig_gpu(A[None])
    dt = time.time() - t0
    assert dt < 1.0, dt
    _check_eig(A, W[0], V[0], int(info[0]))
    print("batch_eig n = %d: %.3f s" % (n, dt))


def test_batch_eig_two_large_matrices_and_the_size_limit():
    import cuadmm_amd
    from tests.helpers import Dev
    rng = np.random.default_rng(5)
    A = np.stack([_eig_family(300, "randn", rng), _eig_family(300, "clustered", rng)])
    W, V, info = batch_eig_gpu(A)
    for i in range(2):
        _check_eig(A[i], W[i], V[i], int(info[i]))
    lib = cuadmm_amd.load()
    big = Dev(shape=(16,)); w2 = Dev(shape=(16,)); i2 = Dev(np.zeros(1, np.int32))
    rc = lib.cuadmm_op_batch_eig(big.ptr, w2.ptr, i2.ptr, 8193, 1, None)       # refused before anything is touched
    assert rc == -1 and b"8192" in lib.cuadmm_last_error()


def test_batch_eig_reference_kats():
    """Spectra hard-coded in the reference tests (test/cusolver_test.hpp:60-63,117-126,178-182)."""
    A4 = np.array([[4, 1, 2, 2], [1, 4, 1, 2], [2, 1, 4, 1], [2, 2, 1, 4]], dtype=float)
    W, V, info = batch_eig_gpu(A4[None])
    assert np.allclose(W[0], [1.38197, 2.45862, 3.61803, 8.54138], atol=1e-5)
    exp = np.array([[-1.0, -0.618034, 0.618034, 1.0], [1.0, -1.18046, -1.18046, 1.0],
                    [-1.0, 1.61803, -1.61803, 1.0], [1.0, 0.847127, 0.847127, 1.0]])
    exp /= np.linalg.norm(exp, axis=1, keepdims=True)
    assert np.allclose(np.abs(V[0].T), np.abs(exp), atol=1e-5)
    W2, _, _ = batch_eig_gpu(np.array([[[2.0, 1.0], [1.0, 3.0]]]))
    assert np.allclose(W2[0], [0.5 * (5 - 5 ** 0.5), 0.5 * (5 + 5 ** 0.5)], atol=1e-12)
    W3, _, _ = batch_eig_gpu(np.array([[[3.0, 1, 2], [1, 3, 1], [2, 1, 3]]]))
    assert np.allclose(W3[0], [1.0, 4 - 3 ** 0.5, 4 + 3 ** 0.5], atol=1e-12)


# ------------------------------------------------------------------------------------------------------------
# Blocks with n > 64: GEMM-only projection through the matrix sign function (psd_large.hip).  The oracle is still the
# LAPACK eigendecomposition; tolerance 1e-12 * ||X||_2-ish per entry (an eigenvalue below 1e-13 ||X||_1 may be
# treated as zero: its contribution to the projection is at most its own size).
# ------------------------------------------------------------------------------------------------------------
def _spectrum_matrix(n, kind, rng):
    if kind == "randn":
        M = rng.standard_normal((n, n)); return (M + M.T) / 2
    if kind == "lowrank":                 # late-ADMM iterate: rank 5 plus indefinite noise at 1e-7
        U = rng.standard_normal((n, 5)); G = rng.standard_normal((n, n))
        return U @ U.T + 1e-7 * (G + G.T)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    if kind == "graded":                  # both signs over 14 decades
        lam = np.concatenate([10.0 ** rng.uniform(-14, 0, n // 2), -10.0 ** rng.uniform(-14, 0, n - n // 2)])
    elif kind == "psd":
        lam = rng.uniform(0.1, 3.0, n)
    elif kind == "nsd":
        lam = -rng.uniform(0.1, 3.0, n)
    elif kind == "clustered":             # eigenvalues +-1 (sign function already converged) and a zero cluster
        lam = np.repeat([1.0, -1.0, 0.0, 2.0], (n + 3) // 4)[:n]
    M = (Q * lam) @ Q.T
    return (M + M.T) / 2


@pytest.mark.parametrize("n", [65, 100, 128, 129, 200, 270, 410, 500])     # 270, 410: padded to 288 / 416 (odd number of 32-wide k-tiles)
@pytest.mark.parametrize("kind", ["randn", "lowrank", "graded", "psd", "nsd", "clustered"])
def test_project_sign_path_spectra(n, kind):
    rng = np.random.default_rng(1000 * n + len(kind))
    M = _spectrum_matrix(n, kind, rng)
    blk = np.array([n], dtype=np.int32)
    bidx = orc.BlockIndex(blk)
    x = bidx.pack([M[None]])
    got = psd_project_gpu(x, blk)
    ref = orc.psd_project_svec(bidx, x)
    nrm = np.linalg.norm(M, 2)
    assert np.max(np.abs(got - ref)) <= 2e-12 * max(nrm, 1e-300) * np.sqrt(2)
    if kind == "psd":
        assert np.max(np.abs(got - x)) <= 2e-12 * nrm * np.sqrt(2)          # P+ is the identity on the cone


def test_project_sign_path_batched_groups_and_zero_block():
    """Several padded sizes in one call (N = 128: n = 65, 100, 128; N = 192: 130, 192; N = 256: 200) mixed with
    register-kernel blocks; a zero block stays exactly zero."""
    blk = np.array([100, 32, 65, 130, 128, 8, 100, 200, 192, 100, 64, 70], dtype=np.int32)
    bidx = orc.BlockIndex(blk)
    x = _rand_svec(blk, 21)
    zero_k = 6
    x[int(bidx.off[zero_k]):int(bidx.off[zero_k + 1])] = 0.0
    got = psd_project_gpu(x, blk)
    ref = orc.psd_project_svec(bidx, x)
    assert np.max(np.abs(got - ref)) <= 2e-12 * 200
    assert np.all(got[int(bidx.off[zero_k]):int(bidx.off[zero_k + 1])] == 0.0)


@pytest.mark.parametrize("blk", [[66, 66, 66, 91, 91, 91, 120, 120, 120], [128], [65, 200, 100, 224], [300, 300]])
def test_project_sign_path_one_launch_variant_is_bit_identical(blk, monkeypatch):
    """A handful of mid-size blocks (PlanarHand_N=1's nine of 66 / 91 / 120 first) run their whole sign iteration in ONE launch
    with per-member barriers (lg_sign_cluster_kernel) instead of ~95 dependent launches: same tile bodies, same slots, same state
    machine -- the projection must not differ by one bit, on easy spectra and on moment-like ones (rank deficient, ~40 steps)."""
    blk = np.array(blk, dtype=np.int32)
    bidx = orc.BlockIndex(blk)
    rng = np.random.default_rng(int(blk.sum()))
    mats = []
    for k, n in enumerate(blk):
        if k % 2 == 0:
            mats.append(_spectrum_matrix(int(n), "randn", rng))
        else:                                                   # moment-matrix-like: rank 3 plus noise at 1e-12
            U = rng.standard_normal((int(n), 3)); G = rng.standard_normal((int(n), int(n)))
            mats.append(U @ U.T + 1e-12 * (G + G.T))
    x = np.concatenate([orc.BlockIndex([m.shape[0]]).pack([m[None]]) for m in mats])
    monkeypatch.setenv("CUADMM_PSD_LG_CLUSTER", "1")          # members on one XCD each: barriers through the shared L2 (checked at run time)
    one = psd_project_gpu(x, blk)
    monkeypatch.setenv("CUADMM_PSD_LG_CLUSTER", "2")          # the same launch with agent-scope release / acquire barriers
    one_agent = psd_project_gpu(x, blk)
    monkeypatch.setenv("CUADMM_PSD_LG_CLUSTER", "0")
    many = psd_project_gpu(x, blk)
    assert np.array_equal(one, many) and np.array_equal(one_agent, many)
    ref = orc.psd_project_svec(bidx, x)
    assert np.max(np.abs(one - ref)) <= 2e-12 * max(np.linalg.norm(m, 2) for m in mats) * np.sqrt(2)


@pytest.mark.parametrize("blk", [[252, 56, 56, 56] + [126] * 10, [66, 130, 300, 91, 140], [100, 200, 330, 450]])
def test_project_sign_path_groups_in_one_launch_are_bit_identical(blk, monkeypatch):
    """One-launch groups of different padded sizes (taha1a: ten blocks of 126 and one of 252) share ONE launch, each with a workspace of
    its own, instead of running one after the other in a shared one (psd_lg_merge): the same tile bodies on the same data -- not one
    bit may differ."""
    blk = np.array(blk, dtype=np.int32)
    bidx = orc.BlockIndex(blk)
    x = _rand_svec(blk, int(blk.sum()))
    monkeypatch.setenv("CUADMM_PSD_LG_MERGE", "1")
    beside = psd_project_gpu(x, blk)
    beside2 = psd_project_gpu(-x, blk)
    monkeypatch.setenv("CUADMM_PSD_LG_MERGE", "0")
    serial = psd_project_gpu(x, blk)
    serial2 = psd_project_gpu(-x, blk)
    assert np.array_equal(beside, serial) and np.array_equal(beside2, serial2)
    ref = orc.psd_project_svec(bidx, x)
    assert np.max(np.abs(beside - ref)) <= 2e-12 * 70


@pytest.mark.parametrize("blk", [[252, 56, 56, 56, 126], [200, 100], [252, 126]])
def test_engine_solves_with_merged_one_launch_groups_leave_the_per_group_bits(blk):
    """The regression test of the one-launch kernel's barrier (csrc/psd_large.hip: lg_member_barrier).  Its XCD-local variant once
    issued a workgroup-scope invalidate that does not drop the L1; stale operand lines were almost always evicted in time, so the
    op-level bit-identity tests passed -- but INSIDE THE ENGINE (the same plan and buffers projection after projection) two groups
    in one launch left the per-group launches' bits in one solve of three.  80 sGS iterations, six solves, must be identical."""
    import cuadmm_amd
    from cuadmm_amd import synthetic
    prob = synthetic.make_synthetic(blk, cons_per_block=5, dense_C=True)

    def run(merge):
        s = cuadmm_amd.SDPSolver(verbose=False, options={"psd_lg_merge": merge})
        s.init_problem(cuadmm_amd.Problem(prob.vec_len, prob.con_num, prob.blk, prob.At_col_ptrs, prob.At_row_ids, prob.At_vals,
                                          prob.b_idx, prob.b_vals, prob.C_idx, prob.C_vals))
        s.solve(80, 0.0, 0, 50, 100, 11000, 1.05)
        return np.array(s.info_arr("pobj")), np.array(s.info_arr("errRd"))
    ref = run(0)
    for _ in range(6):
        got = run(1)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_project_one_workgroup_kernels_third_lds_matrix_is_bit_identical(monkeypatch):
    """33 <= n <= 64 with few blocks of a class (a moment relaxation: pendulum N = 80 has 80 of n = 55): the one-workgroup kernel
    with the next iterate stored beside the current one and the statistics only where the schedule reads them
    (psd_sign_lds_body<NP, TRIPLE>) against the two-matrix variant -- same decisions, same iterates, not one bit of difference."""
    rng = np.random.default_rng(5)
    blk = np.array([55] * 40 + [45] * 30 + [64, 33, 48, 49], np.int32)
    bidx = orc.BlockIndex(blk)
    x = rng.standard_normal(int(bidx.off[-1]))
    for k in range(0, blk.size, 3):                             # moment-matrix-like: rank 3 plus noise at 1e-12 (~40 steps)
        n = int(blk[k]); U = rng.standard_normal((n, 3)); G = rng.standard_normal((n, n))
        x[int(bidx.off[k]):int(bidx.off[k + 1])] = orc.BlockIndex([n]).pack([(U @ U.T + 1e-12 * (G + G.T))[None]])
    monkeypatch.setenv("CUADMM_PSD_LDS_TRIPLE", "1")
    a = psd_project_gpu(x, blk)
    monkeypatch.setenv("CUADMM_PSD_LDS_TRIPLE", "0")
    b = psd_project_gpu(x, blk)
    assert np.array_equal(a, b)
    assert np.max(np.abs(a - orc.psd_project_svec(bidx, x))) <= 1e-12 * 64


def test_project_sign_path_full_size_properties():
    """BASELINE config 3 size (one block of n = 2000): oracle parity, idempotence, Moreau decomposition, complementarity."""
    n = 2000
    blk = np.array([n], dtype=np.int32)
    x = _rand_svec(blk, 22)
    p1 = psd_project_gpu(x, blk)
    pm = psd_project_gpu(-x, blk)
    p2 = psd_project_gpu(p1, blk)
    scale = 70.0                                                            # ||X||_2 of this input ~ 2 sqrt(n) / sqrt(2)
    assert np.max(np.abs(p2 - p1)) <= 1e-12 * scale
    assert np.max(np.abs((p1 - pm) - x)) <= 1e-12 * scale
    assert abs(np.dot(p1, pm)) <= 1e-10 * np.dot(x, x)
    ref = orc.psd_project_svec(orc.BlockIndex(blk), x)
    assert np.max(np.abs(p1 - ref)) <= 1e-12 * scale


def test_project_sign_path_beyond_the_old_fence_properties():
    """One block of n = 5000 (rounds 1-3 refused blocks above 4000; Xsyevd has no such fence, include/cuadmm/cusolver.h:76-95):
    the size-independent properties of a projection -- idempotence, Moreau decomposition X = P(X) - P(-X), complementarity."""
    n = 5000
    blk = np.array([n], dtype=np.int32)
    x = _rand_svec(blk, 23)
    p1 = psd_project_gpu(x, blk)
    pm = psd_project_gpu(-x, blk)
    p2 = psd_project_gpu(p1, blk)
    scale = 2.0 * np.sqrt(n) / np.sqrt(2.0)                                 # ~ ||X||_2 of this input
    assert np.max(np.abs(p2 - p1)) <= 1e-12 * scale
    assert np.max(np.abs((p1 - pm) - x)) <= 1e-12 * scale
    assert abs(np.dot(p1, pm)) <= 1e-10 * np.dot(x, x)
    assert np.dot(p1, p1) > 0.2 * np.dot(x, x)


def test_project_sign_path_flags_non_finite_input():
    import cuadmm_amd
    blk = np.array([100, 16], dtype=np.int32)
    x = _rand_svec(blk, 23)
    x[17] = np.nan
    with pytest.raises(cuadmm_amd.CuadmmError):
        psd_project_gpu(x, blk)


@pytest.mark.parametrize("n,count", [(45, 3000), (64, 1500), (33, 2000), (28, 4000)])
def test_project_mid_sizes_in_bulk_properties(n, count):
    """BASELINE config 4 sizes in bulk (several workgroups / wavefronts per CU at once): Moreau decomposition,
    idempotence, complementarity, and a spot check against the oracle."""
    blk = np.full(count, n, dtype=np.int32)
    bidx = orc.BlockIndex(blk)
    x = _rand_svec(blk, 31 + n)
    p1 = psd_project_gpu(x, blk)
    pm = psd_project_gpu(-x, blk)
    p2 = psd_project_gpu(p1, blk)
    scale = np.max(np.abs(x)) * n
    assert np.max(np.abs(p2 - p1)) <= 1e-12 * scale
    assert np.max(np.abs((p1 - pm) - x)) <= 1e-12 * scale
    assert abs(np.dot(p1, pm)) <= 1e-10 * np.dot(x, x)
    for k in np.random.default_rng(1).choice(count, 24, replace=False):
        sl = slice(int(bidx.off[k]), int(bidx.off[k + 1]))
        ref = orc.psd_project_svec(orc.BlockIndex([n]), x[sl])
        assert np.max(np.abs(p1[sl] - ref)) <= 1e-12 * scale


@pytest.mark.parametrize("wave4_min", ["1", "1024"])      # 32 < n <= 64: one wavefront per block | one workgroup per block
@pytest.mark.parametrize("kind", ["randn", "lowrank", "graded", "psd", "nsd", "clustered"])
def test_project_every_mid_size_one_wavefront_per_block(kind, wave4_min, monkeypatch):
    """Every size 9 ... 64 (the one-wavefront-per-block sign kernels of psd_sign_wave.h, NT = 1 ... 4: column-pair svec loads,
    odd sizes, the n = 15 / 16, 31 / 32 and 63 / 64 corners of the pairing) on the spectra families of the sign path, three
    blocks per size in one call, plus an exactly zero block."""
    monkeypatch.setenv("CUADMM_PSD_WAVE4_MIN", wave4_min)
    sizes = np.repeat(np.arange(9, 65), 3)
    rng = np.random.default_rng(77 + len(kind))
    sizes = sizes[rng.permutation(sizes.size)]
    blk = sizes.astype(np.int32)
    bidx = orc.BlockIndex(blk)
    mats = [_spectrum_matrix(int(n), kind, rng) for n in sizes]
    zero_k = 5
    mats[zero_k] = np.zeros_like(mats[zero_k])
    x = np.concatenate([orc.BlockIndex([M.shape[0]]).pack([M[None]]) for M in mats])
    got = psd_project_gpu(x, blk)
    ref = orc.psd_project_svec(bidx, x)
    for k, M in enumerate(mats):
        sl = slice(int(bidx.off[k]), int(bidx.off[k + 1]))
        nrm = max(np.linalg.norm(M, 2), 1e-300)
        assert np.max(np.abs(got[sl] - ref[sl])) <= 2e-12 * nrm * np.sqrt(2), (k, M.shape[0])
    assert np.all(got[int(bidx.off[zero_k]):int(bidx.off[zero_k + 1])] == 0.0)


# ------------------------------------------------------------------------------------------------------------
# The register eigensolver (psd_small_reg.h: Householder + implicit QL) as a projection and as cuadmm_op_batch_eig, and the workgroup
# eigensolver below n = 129, on the spectra families -- by default they only ever see hard spectra at n = 5.
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["randn", "lowrank", "graded", "psd", "nsd", "clustered"])
def test_project_every_mid_size_register_eigensolver(kind):
    """test_project_every_mid_size_one_wavefront_per_block with psd_n16 = 0, psd_n32 = 0, psd_mid = 1: every size 9 ... 64 through the
    register eigensolver (NMAX = 16, 32, 64), which a rank mask and cuadmm_lambda_min use as well; same inputs, same tolerance."""
    sizes = np.repeat(np.arange(9, 65), 3)
    rng = np.random.default_rng(77 + len(kind))
    sizes = sizes[rng.permutation(sizes.size)]
    blk = sizes.astype(np.int32)
    bidx = orc.BlockIndex(blk)
    mats = [_spectrum_matrix(int(n), kind, rng) for n in sizes]
    zero_k = 5
    mats[zero_k] = np.zeros_like(mats[zero_k])
    x = np.concatenate([orc.BlockIndex([M.shape[0]]).pack([M[None]]) for M in mats])
    got = psd_project_gpu(x, blk, opts={"psd_n16": 0, "psd_n32": 0, "psd_mid": 1})
    ref = orc.psd_project_svec(bidx, x)
    for k, M in enumerate(mats):
        sl = slice(int(bidx.off[k]), int(bidx.off[k + 1]))
        nrm = max(np.linalg.norm(M, 2), 1e-300)
        assert np.max(np.abs(got[sl] - ref[sl])) <= 2e-12 * nrm * np.sqrt(2), (k, M.shape[0])
    assert np.all(got[int(bidx.off[zero_k]):int(bidx.off[zero_k + 1])] == 0.0)


@pytest.mark.parametrize("kind", ["randn", "lowrank", "graded", "psd", "nsd", "clustered", "rank1"])
def test_project_tiny_blocks_spectra(kind):
    """n = 1 ... 8 (always the register eigensolver), 16 blocks per size permuted into one call: several blocks share a wavefront and
    need different numbers of QL sweeps.  The sign path's families plus rank one, an exactly zero block, the same tolerance per block."""
    sizes = np.repeat(np.arange(1, 9), 16)
    rng = np.random.default_rng(99 + len(kind))
    sizes = sizes[rng.permutation(sizes.size)]
    blk = sizes.astype(np.int32)
    bidx = orc.BlockIndex(blk)
    mats = []
    for n in sizes:
        if kind == "rank1":
            v = rng.standard_normal(int(n)); mats.append(np.outer(v, v) * rng.choice([-1.0, 1.0]))
        else:
            mats.append(_spectrum_matrix(int(n), kind, rng))
    zero_k = int(np.nonzero(sizes == 8)[0][0])
    mats[zero_k] = np.zeros_like(mats[zero_k])
    x = np.concatenate([orc.BlockIndex([M.shape[0]]).pack([M[None]]) for M in mats])
    got = psd_project_gpu(x, blk, opts={})
    ref = orc.psd_project_svec(bidx, x)
    for k, M in enumerate(mats):
        sl = slice(int(bidx.off[k]), int(bidx.off[k + 1]))
        nrm = max(np.linalg.norm(M, 2), 1e-300)
        assert np.max(np.abs(got[sl] - ref[sl])) <= 2e-12 * nrm * np.sqrt(2), (k, M.shape[0])
    assert np.all(got[int(bidx.off[zero_k]):int(bidx.off[zero_k + 1])] == 0.0)


_EIG_KINDS = ["randn", "rank1", "lowrank", "identity", "zero", "diag", "graded", "clustered", "tight"]


@pytest.mark.parametrize("kind", _EIG_KINDS + ["mixed"])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128])
def test_batch_eig_below_the_whole_chip_path_spectra(n, kind):
    """cuadmm_op_batch_eig on the nine families on both sides of every boundary below n = 129: the size classes of the register eigensolver
    (4 | 5, 8 | 9, 16 | 17, 32 | 33, 64) and the workgroup eigensolver with the matrix in LDS (65 ... 128: one, two wavefronts of QL; its HBM
    variant starts at n = 137, beyond the whole-chip path's first size, so this entry point never reaches it).  Three members per call;
    "mixed": three different families, so the members' sweep counts differ."""
    rng = np.random.default_rng(5000 + 10 * n + len(kind))
    kinds = ("graded", "rank1", "clustered") if kind == "mixed" else (kind,) * 3
    A = np.stack([_eig_family(n, k, rng) for k in kinds])
    W, V, info = batch_eig_gpu(A)
    for i in range(3):
        _check_eig(A[i], W[i], V[i], int(info[i]))
