"""The hand-placed closed-block problems of tests/_closed_cases.py hold the structure they were written for (CPU only).

Every fact is recomputed from the arrays a solver receives, not from the builder's row lists: what the engine's record of a block
(ClosedRec, psd_fuse.h) will contain -- rows nk, nonzeros nnz, the longest row maxlen, the multiplicity of every svec slot
(= the scatter rounds of A^T y), nonzeros on the first and the last slot -- and that the inputs are well conditioned, so that
the parity bounds of tests/test_gpu_closed_edges.py measure the kernels and not the data."""
import numpy as np
import pytest

from oracle import cuadmm_oracle as orc
from tests import _closed_cases as cc


def blocks_of(args):
    """-> per block: list of (constraint id, local slots, values), constraint ids ascending"""
    L, m, blk, cp, rows, vals = args[:6]
    b64 = blk.astype(np.int64)
    off = np.concatenate([[0], np.cumsum(b64 * (b64 + 1) // 2)])
    assert off[-1] == L and cp.size == m + 1 and cp[-1] == rows.size == vals.size
    out = [[] for _ in blk]
    for j in range(m):
        r = rows[cp[j]:cp[j + 1]].astype(np.int64)
        assert r.size > 0, "constraint %d is empty" % j
        k = int(np.searchsorted(off, r[0], side="right")) - 1
        assert np.all((r >= off[k]) & (r < off[k + 1])), "constraint %d leaves block %d" % (j, k)
        assert np.all(np.diff(r) > 0), "constraint %d repeats a slot or is not sorted" % j
        out[k].append((j, r - off[k], vals[cp[j]:cp[j + 1]]))
    return out


def facts(args):
    blk = args[2]
    per = []
    for k, rws in enumerate(blocks_of(args)):
        n = int(blk[k])
        L = n * (n + 1) // 2
        mult = np.zeros(L, int)
        for _, sl, _ in rws:
            mult[sl] += 1
        per.append({"n": n, "L": L, "nk": len(rws), "nnz": int(mult.sum()), "maxlen": max([sl.size for _, sl, _ in rws], default=0),
                    "mult": mult, "rows": rws})
    return per


ALL = sorted(cc.CASES)
STACKED = [nm for nm in ALL if cc.CASES[nm][1] == "stacked"]
RAGGED = [nm for nm in ALL if cc.CASES[nm][1] == "ragged"]


@pytest.mark.parametrize("name", ALL)
def test_limits_of_the_record_hold_and_are_met(name):
    args = cc.case(name)
    per = facts(args)
    structure = cc.CASES[name][1]
    assert sum(f["nk"] > 0 for f in per) >= 256                       # the device-side forest solve starts at 256 trees
    assert all(f["nk"] <= cc.MAX_ROWS and f["nnz"] <= cc.MAX_NNZ for f in per)
    assert max(f["nk"] for f in per) == cc.MAX_ROWS and max(f["nnz"] for f in per) == cc.MAX_NNZ     # both limits met together
    assert any(f["nk"] == cc.MAX_ROWS and f["nnz"] == cc.MAX_NNZ for f in per)
    big = [f for f in per if f["L"] >= 66]                            # n >= 11: the caps for small blocks do not apply
    assert big
    if structure in ("dense", "rowless"):
        assert all(f["maxlen"] == 8 and f["nnz"] == 64 for f in per if f["nk"])
        assert all(f["mult"].max() == 1 for f in big if f["nk"])
        assert all(f["mult"].max() == 2 for f in per if f["nk"] and f["L"] < 64)      # n = 9: 64 nonzeros on 45 slots
    if structure == "rowless":
        gaps = [k for k, f in enumerate(per) if f["nk"] == 0]
        assert len(gaps) == len(per) // 4 and gaps == [k for k in range(len(per)) if cc.is_rowless(k)]
    else:
        assert all(f["nk"] > 0 for f in per)


@pytest.mark.parametrize("name", ALL)
def test_first_and_last_slot_carry_nonzeros(name):
    args = cc.case(name)
    per = facts(args)
    structure = cc.CASES[name][1]
    if structure == "ragged":        # the single-nonzero rows walk over (0,0), (n-1,n-1) and a middle diagonal slot; the long rows hold both ends
        assert any(f["mult"][0] for f in per) and any(f["mult"][f["L"] - 1] for f in per)
        assert all(f["mult"][0] and f["mult"][f["L"] - 1] for f in per if f["nk"] == 8)
    else:
        assert all(f["mult"][0] and f["mult"][f["L"] - 1] for f in per if f["nk"])


@pytest.mark.parametrize("name", STACKED)
def test_stacked_blocks_need_eight_scatter_rounds(name):
    for f in facts(cc.case(name)):
        mult, L, n = f["mult"], f["L"], f["n"]
        assert f["nk"] == 8 and mult[0] == 8 and mult[L - 1] == 8                     # nrounds = 8, on two diagonal slots
        three = np.nonzero(mult == 3)[0]
        assert three.size == 1 and int(three[0]) not in [cc.diag_slot(i) for i in range(n)]
        assert sorted(k for k, (_, sl, _) in enumerate(f["rows"]) if three[0] in sl) == [0, 3, 7]
        assert set(np.unique(mult)) == {0, 1, 3, 8}
        assert f["nnz"] == (64 if L >= 48 else 56)


@pytest.mark.parametrize("name", RAGGED)
def test_ragged_blocks_differ_in_rows_and_lengths(name):
    per = facts(cc.case(name))
    assert [f["nk"] for f in per] == [1 + k % 8 for k in range(len(per))]
    singles_on = set()
    for f in per:
        n, L = f["n"], f["L"]
        lens = [sl.size for _, sl, _ in f["rows"]]
        diag = [cc.diag_slot(i) for i in range(n)]
        assert any(sz == 1 and int(sl[0]) in diag for _, sl, _ in f["rows"] for sz in [sl.size])     # a single nonzero on a diagonal slot
        singles_on |= {("first" if sl[0] == 0 else "last" if sl[0] == L - 1 else "inner") for _, sl, _ in f["rows"] if sl.size == 1 and int(sl[0]) in diag}
        if f["nk"] == 8:
            ll = min(cc.LONG_ROW, L - 1)
            assert sorted(lens) == [1] * 7 + [ll] and f["maxlen"] == ll and f["nnz"] == ll + 7
            assert f["mult"].max() == 2                                              # single rows sit on slots of the long row
        else:
            assert lens[0] == 1 and f["mult"].max() == 1
    assert singles_on == {"first", "last", "inner"}
    long_at = set(int(np.argmax([sl.size for _, sl, _ in f["rows"]])) for f in per if f["nk"] == 8)
    assert len(long_at) >= 4                                                         # the long row is not always the same local row
    assert any(f["nnz"] == 64 and f["maxlen"] == 57 for f in per)


@pytest.mark.parametrize("name", ALL)
def test_every_block_is_well_conditioned(name):
    """cond(A_k A_k^T) <= 1e4: a condition on the INPUTS (the seeds of _closed_cases.CASES were chosen for it)."""
    args = cc.case(name)
    worst = 0.0
    for f in facts(args):
        if not f["nk"]:
            continue
        A = np.zeros((f["nk"], f["L"]))
        for i, (_, sl, v) in enumerate(f["rows"]):
            A[i, sl] = v
        worst = max(worst, float(np.linalg.cond(A @ A.T)))
    print("%s: worst cond(A_k A_k^T) = %.1f" % (name, worst))
    assert worst <= 1e4


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("sw", [0, 5, 1000])          # ADMM only | sGS then the switch | sGS only
def test_oracle_stays_finite(name, sw):
    args = cc.case(name)
    o = orc.OracleSolver().init_problem(orc.Problem(*args))
    info = o.solve(12, 0.0, 0, 50, 100, sw, 1.05)
    for nm in ("errRp", "errRd", "pobj", "dobj", "relgap"):
        a = np.asarray(getattr(info, nm), float)
        assert a.size == 12 and np.all(np.isfinite(a)), nm
    assert np.all(np.isfinite(o.X)) and np.all(np.isfinite(o.y)) and np.all(np.isfinite(o.S))


def test_builder_is_deterministic():
    blk, structure, seed = cc.CASES["ragged-edges"]
    a, b = cc.build(blk, structure, seed), cc.build(blk, structure, seed)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = cc.build(blk, structure, seed + 1)
    assert not np.array_equal(a[5], c[5])
