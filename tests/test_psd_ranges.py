"""The launch-range table of the projection planner (csrc/psd_plan.h: PsdRanges), on the host: which kernel serves which members
under every option that selects one, and the three things derived from the table -- the fused blocks, their partial-sum slots and
the rest index -- through the hook cuadmm_psd_plan_ranges.  Every expected value below is written out by hand.  No device."""
import ctypes as C

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd._lib import check

lib = cuadmm_amd.load()
P = lambda a: a.ctypes.data_as(C.c_void_p)
REG, WG, CHIP, WAVE, LDS = range(5)

BLK = [3, 8, 12, 16, 24, 32, 40, 48, 56, 64, 70, -5]          # block k of this list is "k" in the ids below
IDS = [0, 1, 3, 2, 5, 4, 9, 8, 7, 6]                           # classes ascending, members of a class largest first; 70: batched GEMM


def ranges_of(blk, opts=None, eig_rank=0, tiny_sign=0):
    blk = np.array(blk, np.int32)
    opts = opts or {}
    keys = (C.c_char_p * max(len(opts), 1))(*[k.encode() for k in opts])
    vals = np.array(list(opts.values()) + [0.0], np.float64)
    L = int(sum(n * (n + 1) // 2 if n > 0 else -n for n in blk.tolist()))
    rng, ids, slot, rest, summ = np.full(80, -7, np.int32), np.full(blk.size, -7, np.int32), np.full(blk.size, -7, np.int32), np.full(L, -7, np.int32), np.zeros(6, np.int32)
    check(lib.cuadmm_psd_plan_ranges(P(blk), blk.size, eig_rank, tiny_sign, keys, P(vals), len(opts), P(rng), P(ids), P(slot), P(rest), P(summ)))
    nr, nid, nrest, fusable, fused, sign_min = summ.tolist()
    assert (rng[10 * nr:] == -7).all()
    names = ("cls", "first", "count", "kind", "nt", "occ", "occ_batch", "full", "triple", "maxn")
    return dict(blk=blk.tolist(), L=L, ranges=[dict(zip(names, rng[10 * i:10 * i + 10].tolist())) for i in range(nr)], ids=ids[:nid].tolist(),
                slot=slot.tolist(), rest=rest[:nrest].tolist(), fusable=bool(fusable), fused=fused, sign_min=sign_min)


# (class, first, count, kind, tiles) per range, the members, fusable, and the blocks that own partial-sum slots 0, 1, 2, ...
CASES = {
    "default": (dict(), [(0, 0, 1, REG, 0), (1, 1, 1, REG, 0), (2, 2, 2, WAVE, 1), (3, 4, 2, WAVE, 2), (4, 6, 2, LDS, 4), (4, 8, 2, LDS, 3)],
                IDS, True, [3, 2, 5, 4]),
    "psd_n16=0": (dict(opts={"psd_n16": 0}), [(0, 0, 1, REG, 0), (1, 1, 1, REG, 0), (2, 2, 2, REG, 0), (3, 4, 2, WAVE, 2), (4, 6, 2, LDS, 4), (4, 8, 2, LDS, 3)],
                  IDS, True, [5, 4]),
    "psd_n32=0": (dict(opts={"psd_n32": 0}), [(0, 0, 1, REG, 0), (1, 1, 1, REG, 0), (2, 2, 2, WAVE, 1), (3, 4, 2, REG, 0), (4, 6, 2, LDS, 4), (4, 8, 2, LDS, 3)],
                  IDS, False, [3, 2]),
    "psd_mid=1": (dict(opts={"psd_mid": 1}), [(0, 0, 1, REG, 0), (1, 1, 1, REG, 0), (2, 2, 2, WAVE, 1), (3, 4, 2, WAVE, 2), (4, 6, 4, REG, 0)],
                  IDS, False, [3, 2, 5, 4]),
    "psd_mid=2": (dict(opts={"psd_mid": 2}), [(0, 0, 1, REG, 0), (1, 1, 1, REG, 0), (2, 2, 2, WAVE, 1), (3, 4, 2, WAVE, 2), (4, 6, 2, LDS, 4), (4, 8, 2, LDS, 3)],
                  IDS, True, [3, 2, 5, 4]),
    "psd_wave4_min=1": (dict(opts={"psd_wave4_min": 1}), [(0, 0, 1, REG, 0), (1, 1, 1, REG, 0), (2, 2, 2, WAVE, 1), (3, 4, 2, WAVE, 2), (4, 6, 2, WAVE, 4), (4, 8, 2, WAVE, 3)],
                        IDS, True, [3, 2, 5, 4, 9, 8, 7, 6]),
    "tiny_sign": (dict(tiny_sign=1), [(2, 0, 4, WAVE, 1), (3, 4, 2, WAVE, 2), (4, 6, 2, LDS, 4), (4, 8, 2, LDS, 3)],
                  [3, 2, 1, 0, 5, 4, 9, 8, 7, 6], True, [3, 2, 1, 0, 5, 4]),
    # a rank mask needs eigenvalues: nothing takes a sign kernel, and the block of 70 joins the table (workgroup eigensolver)
    "eig_rank=2": (dict(eig_rank=2), [(0, 0, 1, REG, 0), (1, 1, 1, REG, 0), (2, 2, 2, REG, 0), (3, 4, 2, REG, 0), (4, 6, 4, REG, 0), (5, 10, 1, WG, 0)],
                   IDS + [10], False, []),
}


@pytest.mark.parametrize("name", list(CASES))
def test_ranges_of_the_mixed_list(name):
    kw, want, ids, fusable, slot_owners = CASES[name]
    t = ranges_of(BLK, **kw)
    assert [(r["cls"], r["first"], r["count"], r["kind"], r["nt"] if r["kind"] in (WAVE, LDS) else 0) for r in t["ranges"]] == want
    assert t["ids"] == ids and t["fusable"] == fusable
    assert t["sign_min"] == (2**31 - 1 if name == "eig_rank=2" else 65)
    # the ranges tile [0, PSD blocks below sign_min) in order, and the members are exactly those blocks
    at = 0
    for r in t["ranges"]:
        assert r["first"] == at and r["count"] > 0
        at += r["count"]
        assert r["maxn"] == BLK[t["ids"][r["first"]]] == max(BLK[k] for k in t["ids"][r["first"]:at])
    assert at == len(ids) == sum(1 for n in BLK if 0 < n < t["sign_min"]) and sorted(ids) == [k for k, n in enumerate(BLK) if 0 < n < t["sign_min"]]
    # fused blocks = the members of the one-wavefront ranges, numbered 0 .. k-1 in launch order; the rest index is their complement
    members = [k for r in t["ranges"] if r["kind"] == WAVE for k in t["ids"][r["first"]:r["first"] + r["count"]]]
    assert members == slot_owners and t["fused"] == len(members)
    assert t["slot"] == [members.index(k) if k in members else -1 for k in range(len(BLK))]
    off = np.concatenate([[0], np.cumsum([n * (n + 1) // 2 if n > 0 else -n for n in BLK])])
    assert t["rest"] == [i for k in range(len(BLK)) if k not in members for i in range(off[k], off[k + 1])]
    assert len(t["rest"]) + sum(BLK[k] * (BLK[k] + 1) // 2 for k in members) == t["L"] == off[-1]


def test_occupancies_and_the_third_lds_matrix():
    by_nt = lambda t: {(r["kind"], r["nt"]): r for r in t["ranges"]}
    t = by_nt(ranges_of(BLK, {"psd_wave4_min": 1}))
    assert [(t[WAVE, nt]["occ"], t[WAVE, nt]["occ_batch"]) for nt in (1, 2, 3, 4)] == [(8, 8), (4, 4), (2, 2), (1, 1)]
    t = by_nt(ranges_of(BLK, {"psd_w32_occ": 3}))
    assert (t[WAVE, 2]["occ"], t[WAVE, 2]["occ_batch"]) == (3, 4)
    t = by_nt(ranges_of(BLK, {"psd_cu_occ": 3}))
    assert (t[WAVE, 2]["occ"], t[WAVE, 2]["occ_batch"]) == (4, 3)
    assert by_nt(ranges_of(BLK))[LDS, 4]["triple"] == 1 and by_nt(ranges_of(BLK))[LDS, 3]["triple"] == 1
    assert by_nt(ranges_of(BLK, {"psd_lds_triple": 0}))[LDS, 4]["triple"] == 0
    assert by_nt(ranges_of([40] * 257))[LDS, 3]["triple"] == 0          # more than 256 blocks: the third matrix would cost occupancy
    assert ranges_of([40] * 1024)["ranges"][0]["kind"] == WAVE and ranges_of([40] * 1023)["ranges"][0]["kind"] == LDS   # psd_wave4_min = 1024
    assert [r["kind"] for r in ranges_of(BLK, {"psd_mid": 2, "psd_wave4_min": 1})["ranges"][-2:]] == [LDS, LDS]   # psd_mid = 2 overrides the count
    assert ranges_of([70, 100, 120], {"psd_sign_min": 101})["ids"] == [1, 0] and ranges_of([70, 100, 120], {"psd_sign_min": 101})["ranges"][0]["kind"] == WG


def test_full_flag():
    """full: every member of a one-wavefront range fills its tile exactly (n = 16 tiles)."""
    assert [(r["kind"], r["nt"], r["count"], r["full"]) for r in ranges_of([32] * 5)["ranges"]] == [(WAVE, 2, 5, 1)]
    assert [(r["kind"], r["nt"], r["count"], r["full"]) for r in ranges_of([48] * 3, {"psd_wave4_min": 1})["ranges"]] == [(WAVE, 3, 3, 1)]
    assert [(r["kind"], r["nt"], r["count"], r["full"]) for r in ranges_of([48] * 3)["ranges"]] == [(LDS, 3, 3, 0)]   # a flag of the one-wavefront ranges only
    assert [(r["nt"], r["full"]) for r in ranges_of([64, 48, 64, 47, 16, 32, 31], {"psd_wave4_min": 1})["ranges"]] == [(1, 1), (2, 0), (4, 1), (3, 0)]
    assert all(r["full"] == 0 for r in ranges_of(BLK, {"psd_wave4_min": 1})["ranges"])
