"""The inputs of tests/test_gpu_lead_solve.py, checked without a GPU: every generated A, factored with the tail the GPU case forces,
must have the leading elimination forest that case was built for (the minimum-degree ordering decides it, not the generator alone),
and must be so well conditioned that plain float64 substitution is within 1e-13 of the extended-precision reference."""
import numpy as np
import pytest

from tests import helpers as H

# LDS a tree needs with its stream resident (lead_solve.hip, build_core): 24 bytes per node and 12 per nonzero of L11, to the first order
NEED = lambda fo: 24 * fo["sizes"] + 12 * fo["nnz11"]


@pytest.fixture(scope="module")
def factors():
    cache = {}

    def get(name):
        if name not in cache:
            A, k, marks = H.lead_case(name)
            cache[name] = (H.Factor(A, k), marks)
        return cache[name]
    yield get
    for f, _ in cache.values():
        f.close()


def test_small_trees(factors):
    fo = factors("small")[0].forest()
    assert fo["sizes"].size == 240 and fo["sizes"].min() >= 20 and fo["sizes"].max() <= 300
    assert NEED(fo).max() < 15 * 1024                       # every tree below the 16 KB bound of a shared workgroup
    assert fo["tail_rows"].max() <= 128


def test_mixed_trees(factors):
    fo = factors("mixed")[0].forest()
    need = NEED(fo)
    assert fo["sizes"].size == 65 and fo["sizes"].max() == 6000          # at the sweeps' limit of 6 144 nodes
    assert (need < 3 * 1024).sum() >= 10                                   # small under every bound (4, 8, 16 KB)
    assert ((need > 20 * 1024) & (need < 150 * 1024)).sum() >= 4          # resident, a workgroup of their own
    assert (need > 170 * 1024).sum() == 1                                  # beyond one workgroup's LDS: streaming
    assert ((need > 5 * 1024) & (need < 7 * 1024)).sum() + ((need > 9 * 1024) & (need < 15 * 1024)).sum() >= 4   # change class with the bound


def test_micro_trees(factors):
    fo = factors("micro")[0].forest()
    assert (fo["sizes"] == 1).sum() == 5000 and (fo["sizes"] == 2).sum() == 4500 and (fo["sizes"] > 2).sum() == 4
    assert fo["sizes"].max() == 300


def test_deep_forest(factors):
    fo = factors("deep")[0].forest()
    h = fo["height"]
    tree_height = np.zeros(fo["sizes"].size, np.int64)
    np.maximum.at(tree_height, fo["tree_of"], h)
    assert fo["sizes"].size == 48
    assert (tree_height > 100).sum() == 8 and tree_height.max() == 500    # the chains: cut by tops at height 8 and 32
    assert (tree_height <= 8).sum() >= 1                                   # trees whose top is empty at either cut
    assert ((tree_height > 8) & (tree_height <= 32)).sum() >= 1           # cut at 8, whole at 32
    assert h.max() < 100000                                                # "a level above every node's height" of the GPU case


@pytest.mark.parametrize("rows,k", [(127, 256), (128, 256), (129, 256), (2000, 2048)])
def test_long_tail_columns(factors, rows, k):
    f, marks = factors("long%d" % rows)
    fo = f.forest()
    ip = np.empty(f.m, np.int64)
    ip[f.perm] = np.arange(f.m)
    marked, lonely = ip[marks["marked"]], ip[marks["lonely"]]
    assert f.k == k and marked < f.n1 and lonely < f.n1                  # both are leading columns
    assert fo["tail_rows"][marked] == rows and fo["tail_rows"][lonely] == 0
    others = np.delete(fo["tail_rows"], marked)
    assert others.max() <= 100                                             # the marked column alone decides n_long
    assert (fo["tail_rows"] > 128).sum() == (1 if rows > 128 else 0)


def test_block_diagonal_forest(factors):
    f = factors("forest")[0]
    fo = f.forest()
    assert f.k == 0 and fo["sizes"].size == 400 and fo["sizes"].max() == 64 and fo["sizes"].min() == 1


@pytest.mark.parametrize("name", ["small", "mixed", "micro", "deep", "long127", "long128", "long129", "long2000", "forest"])
def test_inputs_are_well_conditioned(factors, name):
    f = factors(name)[0]
    ax, asmc, b = H.lead_vectors(f.m, 1)
    for isig in (0.7, 1e-6, 1e6):
        xr = f.solve_ref(H.lead_rhs(ax[0], asmc[0], b[0], isig), np.longdouble)
        x64 = f.solve_ref(H.lead_rhs(ax[0], asmc[0], b[0], isig, np.float64), np.float64)
        e64 = float(np.linalg.norm((x64 - xr).astype(np.float64)) / np.linalg.norm(xr.astype(np.float64)))
        assert e64 <= 1e-13, (name, isig, e64)
