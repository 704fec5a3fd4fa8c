"""The group table of the batched-GEMM sign path (csrc/psd_large.hip: SignPsd::build_host, lg_small_tiles, lg_path), on the host, through the
hook cuadmm_psd_sign_groups: which padded size, tile, decision and launch variant a list of blocks gets under every option that selects
one.  Every expected row below is written out by hand.  No device.

A row: (N, members, merged, slot, tile, tiles per member, decision kernel, one-launch kernel, spread, one-launch grid, super-block order,
fused).  The rules the rows were worked out from:
  pad      N = n rounded up to 64; on 32-wide tiles, when every member fits N - 32 (and N - 32 >= 128), N - 32 (psd_lg_pad32)
  tile     32 when N >= 128 and members * nb64 (nb64 + 1) / 2 < 1300 with nb64 = N / 64 (integer division), else 64 (psd_lg_tile forces one)
  tiles    nb (nb + 1) / 2 with nb = N / tile
  decision a kernel of its own above 300 tiles (psd_lg_decide = 1 | 2 forces inline | kernel)
  cluster  one launch for the whole iteration: 32-wide tiles, inline decision, members * tiles <= psd_lg_cluster_wgs (224)
  spread   ceil(members / 8) * tiles > 96; grid = members * tiles when spread, else 8 * ceil(members / 8) * tiles
  merged   two to four one-launch groups with N <= 512 whose workgroups together stay within psd_lg_cluster_wgs share ONE launch
  chunks   a group holds at most max(1, psd_sign_ws_mb MiB / (32 N^2 bytes)) members, N the padded size BEFORE the shrink
"""
import ctypes as C

import numpy as np
import pytest

import cuadmm_amd
from cuadmm_amd._lib import check
from tests import helpers as H

lib = cuadmm_amd.load()
P = lambda a: a.ctypes.data_as(C.c_void_p)


def groups_of(blk, opts=None, cap=256):
    blk = np.array(blk, np.int32)
    keys, vals, n = H.opt_pairs(opts or {})
    out = np.full(12 * cap + 12, -7, np.int32)
    ng = C.c_int(-1)
    check(lib.cuadmm_psd_sign_groups(P(blk), blk.size, keys, P(vals), n, P(out), cap, C.byref(ng)))
    assert (out[12 * ng.value:] == -7).all()
    return [tuple(out[12 * i:12 * i + 12].tolist()) for i in range(ng.value)]


T64, DEC = {"psd_lg_tile": 64}, {"psd_lg_decide": 2}
MULTI = {"psd_lg_cluster": 0}

#                 N  cnt mrg slot tile ntiles dec clu spr  grid  sb fused
R65_64 = (128, 1, 0, 0, 64, 3, 0, 0, 0, 24, 0, 1)
R65_32 = (128, 1, 0, 0, 32, 10, 0, 0, 0, 80, 0, 1)
R270_32 = (288, 1, 0, 0, 32, 45, 0, 0, 0, 360, 0, 1)
R2x128_32 = (128, 2, 0, 0, 32, 10, 0, 0, 0, 80, 0, 1)
R720 = (736, 1, 0, 0, 32, 276, 0, 0, 1, 276, 1, 0)


def _with(row, **kw):
    names = ("N", "count", "merged", "slot", "tile", "ntiles", "decide", "cluster", "spread", "grid", "sb", "fused")
    d = dict(zip(names, row))
    d.update(kw)
    return tuple(d[k] for k in names)


# every (blk, opts) pair of tests/test_gpu_sign_variants.py: (variant or test, blk) -> rows
GPU_CASES = [
    # 64-wide tiles, multi-launch, inline decision: forced tile, hence no shrink and no one-launch kernel
    (H.SIGN_VARIANTS["tile64_inline"]["opts"], [65], [R65_64]),
    (H.SIGN_VARIANTS["tile64_inline"]["opts"], [129], [(192, 1, 0, 0, 64, 6, 0, 0, 0, 48, 0, 1)]),
    (H.SIGN_VARIANTS["tile64_inline"]["opts"], [100, 100, 128], [(128, 3, 0, 0, 64, 3, 0, 0, 0, 24, 0, 1)]),
    # ... with the decision kernel
    (H.SIGN_VARIANTS["tile64_decide"]["opts"], [65], [_with(R65_64, decide=1)]),
    (H.SIGN_VARIANTS["tile64_decide"]["opts"], [129, 192], [(192, 2, 0, 0, 64, 6, 1, 0, 0, 48, 0, 1)]),
    # 32-wide tiles, multi-launch: 65 -> 128 (96 would be below 128), 270 -> 320 -> 288 (nine tiles per side), 130 and 192 -> 192
    (H.SIGN_VARIANTS["tile32_inline"]["opts"], [65], [R65_32]),
    (H.SIGN_VARIANTS["tile32_inline"]["opts"], [270], [R270_32]),
    (H.SIGN_VARIANTS["tile32_inline"]["opts"], [130, 192], [(192, 2, 0, 0, 32, 21, 0, 0, 0, 168, 0, 1)]),
    (H.SIGN_VARIANTS["tile32_decide"]["opts"], [65], [_with(R65_32, decide=1)]),
    (H.SIGN_VARIANTS["tile32_decide"]["opts"], [270], [_with(R270_32, decide=1)]),
    # the default path between the one-launch kernel (<= 224 workgroups) and the decision kernel (> 300 tiles): 720 -> 768 -> 736
    (H.SIGN_VARIANTS["default_window"]["opts"], [720], [R720]),
    (H.SIGN_VARIANTS["default_window"]["opts"], [768], [(768, 1, 0, 0, 32, 300, 0, 0, 1, 300, 1, 0)]),
    # the same two sizes with the decision kernel forced (test_slots_beyond_256_carry_the_decision)
    (DEC, [720], [_with(R720, decide=1)]),
    (DEC, [768], [(768, 1, 0, 0, 32, 300, 1, 0, 1, 300, 1, 0)]),
    # 800 -> 832 -> 800: 325 tiles, the decision inline only because it is forced
    (H.SIGN_VARIANTS["inline_forced"]["opts"], [800], [(800, 1, 0, 0, 32, 325, 0, 0, 1, 325, 1, 0)]),
    # super-block order (one member, >= 16 tiles per side): 512 = 16 x 32; 520 -> 576 -> 544 = 17 x 32; 1024 = 16 x 64; 1030 -> 1088 = 17 x 64
    (H.SIGN_VARIANTS["superblock32"]["opts"], [512], [(512, 1, 0, 0, 32, 136, 0, 0, 1, 136, 1, 1)]),
    (H.SIGN_VARIANTS["superblock32"]["opts"], [520], [(544, 1, 0, 0, 32, 153, 0, 0, 1, 153, 1, 0)]),
    (H.SIGN_VARIANTS["superblock64"]["opts"], [1024], [(1024, 1, 0, 0, 64, 136, 0, 0, 1, 136, 1, 0)]),
    (H.SIGN_VARIANTS["superblock64"]["opts"], [1030], [(1088, 1, 0, 0, 64, 153, 0, 0, 1, 153, 1, 0)]),
    # no shrink: 270 stays at 320 (55 tiles), 410 at 448 (105 tiles: more than an XCD's 96 workgroups, spread); both in one launch
    (H.SIGN_VARIANTS["no_pad32"]["opts"], [270], [(320, 1, 0, 0, 32, 55, 0, 1, 0, 440, 0, 1)]),
    (H.SIGN_VARIANTS["no_pad32"]["opts"], [410], [(448, 1, 0, 0, 32, 105, 0, 1, 1, 105, 0, 1)]),
    # 1 MiB of workspace: 128 x 128 x 32 bytes = 0.5 MiB per member -> chunks of 2, 2, 1, each a one-launch group: merged, slots 1, 2, 3
    (H.SIGN_WS_CHUNKS["opts"], [100] * 5, [(128, 2, 1, 1, 32, 10, 0, 1, 0, 80, 0, 1), (128, 2, 1, 2, 32, 10, 0, 1, 0, 80, 0, 1), (128, 1, 1, 3, 32, 10, 0, 1, 0, 80, 0, 1)]),
    # 192 x 192 x 32 bytes = 1.125 MiB > 1 MiB: 1 MiB / per = 0 -> one member per group all the same; 150 fits 160
    (H.SIGN_WS_CHUNKS["opts"], [150] * 3, [(160, 1, 1, s, 32, 15, 0, 1, 0, 120, 0, 1) for s in (1, 2, 3)]),
    # no polling / polling: 65 and 100 share N = 128, 270 alone at 288
    (H.SIGN_NO_POLL["opts"], H.SIGN_NO_POLL["blk"], [R2x128_32, R270_32]),
    (H.SIGN_NO_POLL["opts_poll"], H.SIGN_NO_POLL["blk"], [R2x128_32, R270_32]),
    # the step cap changes no row
    (H.SIGN_STEP_CAP[0][0], H.SIGN_STEP_CAP[0][1], [R2x128_32, R270_32]),
    (dict(H.SIGN_STEP_CAP[0][0], psd_sign_maxsteps=13), H.SIGN_STEP_CAP[0][1], [R2x128_32, R270_32]),
    (H.SIGN_STEP_CAP[1][0], H.SIGN_STEP_CAP[1][1], [_with(R2x128_32, cluster=1)]),
    (dict(H.SIGN_STEP_CAP[1][0], psd_sign_maxsteps=13), H.SIGN_STEP_CAP[1][1], [_with(R2x128_32, cluster=1)]),
    # non-finite input and the zero block
    (H.SIGN_NON_FINITE[0][0], H.SIGN_NON_FINITE[0][1], [R2x128_32]),
    (H.SIGN_NON_FINITE[1][0], H.SIGN_NON_FINITE[1][1], [(128, 2, 0, 0, 64, 3, 0, 0, 0, 24, 0, 1)]),
    (H.SIGN_NON_FINITE[2][0], H.SIGN_NON_FINITE[2][1], [R720]),
    (H.SIGN_ZERO_BLOCK[0][0], H.SIGN_ZERO_BLOCK[0][1], [(128, 2, 0, 0, 64, 3, 0, 0, 0, 24, 0, 1)]),
    (H.SIGN_ZERO_BLOCK[1][0], H.SIGN_ZERO_BLOCK[1][1], [R2x128_32]),
    (H.SIGN_ZERO_BLOCK[2][0], H.SIGN_ZERO_BLOCK[2][1], [_with(R2x128_32, decide=1)]),
    # the mixed call: 65 -> 128 and 130, 130 -> 192 -> 160 are one-launch groups of 10 + 30 workgroups: merged, first; 700, 700 -> 704 (672 is
    # too small): 2 x 253 tiles, multi-launch, inline; 40 and 8 are not on this path
    (H.SIGN_MIXED_CALL["opts"], H.SIGN_MIXED_CALL["blk"],
     [(128, 1, 1, 1, 32, 10, 0, 1, 0, 80, 0, 1), (160, 2, 1, 2, 32, 15, 0, 1, 0, 120, 0, 1), (704, 2, 0, 0, 32, 253, 0, 0, 1, 506, 0, 0)]),
]


@pytest.mark.parametrize("case", range(len(GPU_CASES)))
def test_every_gpu_case_reaches_the_variant_it_names(case):
    opts, blk, want = GPU_CASES[case]
    assert groups_of(blk, opts) == want


def test_the_gpu_case_table_is_complete():
    """every (blk, opts) pair the GPU tests run has a hand-written row above, and no GPU case raises psd_lg_cluster_wgs"""
    have = {(tuple(sorted(o.items())), tuple(b)) for o, b, _ in GPU_CASES}
    need = [(v["opts"], b) for v in H.SIGN_VARIANTS.values() for b in v["blks"]]
    need += [(H.SIGN_WS_CHUNKS["opts"], b) for b in H.SIGN_WS_CHUNKS["blks"]]
    need += [(H.SIGN_NO_POLL["opts"], H.SIGN_NO_POLL["blk"]), (H.SIGN_NO_POLL["opts_poll"], H.SIGN_NO_POLL["blk"]), (H.SIGN_MIXED_CALL["opts"], H.SIGN_MIXED_CALL["blk"])]
    need += H.SIGN_STEP_CAP + H.SIGN_NON_FINITE + H.SIGN_ZERO_BLOCK
    for o, b in need:
        assert (tuple(sorted(o.items())), tuple(b)) in have, (o, b)
        assert "psd_lg_cluster_wgs" not in o
    # the multi-launch variants are multi-launch (the parity of the step count selects the final product's operand), the others one launch
    for v in H.SIGN_VARIANTS.values():
        for b in v["blks"]:
            assert all((row[7] == 0) == v["multi"] for row in groups_of(b, v["opts"])), (v["opts"], b)


def test_default_table_where_the_three_paths_meet():
    """one block: 640 is the last size of the one-launch kernel (210 workgroups <= 224), 641 ... 768 run launch by launch with the decision
    inline (231 ... 300 tiles), 769 (-> 800, 325 tiles) takes the decision kernel"""
    assert groups_of([640]) == [(640, 1, 0, 0, 32, 210, 0, 1, 1, 210, 1, 0)]
    assert groups_of([641]) == [(672, 1, 0, 0, 32, 231, 0, 0, 1, 231, 1, 0)]
    assert groups_of([768]) == [(768, 1, 0, 0, 32, 300, 0, 0, 1, 300, 1, 0)]
    assert groups_of([769]) == [(800, 1, 0, 0, 32, 325, 1, 0, 1, 325, 1, 0)]
    assert groups_of([800]) == [(800, 1, 0, 0, 32, 325, 1, 0, 1, 325, 1, 0)]           # what psd_lg_decide = 1 overrides in the GPU test


def test_default_tile_changes_between_433_and_434_blocks_of_100():
    """N = 128: three 64-wide tiles per member; 433 x 3 = 1299 < 1300 keeps the 32-wide tiles, 434 x 3 = 1302 does not"""
    assert groups_of([100] * 433) == [(128, 433, 0, 0, 32, 10, 0, 0, 1, 4330, 0, 1)]
    assert groups_of([100] * 434) == [(128, 434, 0, 0, 64, 3, 0, 0, 1, 1302, 0, 1)]


def test_shrink_follows_the_chunk_not_the_class():
    """217 blocks of 150 (N = 192: six 64-wide tiles each): as ONE group 6 x 217 = 1302 tiles take the 64-wide tiling, which cannot shrink;
    in chunks of one (psd_sign_ws_mb = 1) every chunk is on 32-wide tiles and shrinks to 160.  The remainder chunk is never larger than
    the others and the tile rule is monotone in the count, so its count alone cannot veto a shrink the full chunks allow: the two
    cases here are what the count can change.  Of the 217 one-launch groups the first four share a launch."""
    assert groups_of([150] * 217) == [(192, 217, 0, 0, 64, 6, 0, 0, 1, 1302, 0, 1)]
    one = (160, 1, 0, 0, 32, 15, 0, 1, 0, 120, 0, 1)
    assert groups_of([150] * 217, {"psd_sign_ws_mb": 1}) == [_with(one, merged=1, slot=s) for s in (1, 2, 3, 4)] + [one] * 213
    assert groups_of([150] * 216) == [(160, 216, 0, 0, 32, 15, 0, 0, 1, 3240, 0, 1)]     # 1296 < 1300: one group, shrunk
    # chunks of two with a remainder of one: 2, 2, 1 (the GPU case) and the even split
    assert [r[1] for r in groups_of([100] * 5, {"psd_sign_ws_mb": 1})] == [2, 2, 1]
    assert [r[1] for r in groups_of([100] * 4, {"psd_sign_ws_mb": 1})] == [2, 2]


def test_pad32_off_and_on():
    assert groups_of([270]) == [(288, 1, 0, 0, 32, 45, 0, 1, 0, 360, 0, 1)]
    assert groups_of([270], {"psd_lg_pad32": 0}) == [(320, 1, 0, 0, 32, 55, 0, 1, 0, 440, 0, 1)]
    assert groups_of([410]) == [(416, 1, 0, 0, 32, 91, 0, 1, 0, 728, 0, 1)]
    # 2000 -> 2048 -> 2016 = 63 x 32: 2016 tiles; 2048 = 64 x 32: 2080 tiles
    assert groups_of([2000]) == [(2016, 1, 0, 0, 32, 2016, 1, 0, 1, 2016, 1, 0)]
    assert groups_of([2000], {"psd_lg_pad32": 0}) == [(2048, 1, 0, 0, 32, 2080, 1, 0, 1, 2080, 1, 0)]


def test_cluster_wgs_bounds_the_one_launch_kernel():
    """n = 100: ten 32-wide tiles per member.  8 workgroups: not even one member; 16: one member, not two.  (Host only: a GPU test never
    changes this option -- the kernel's barriers rely on a co-resident grid.)"""
    one, two = (128, 1, 0, 0, 32, 10, 0, 0, 0, 80, 0, 1), (128, 2, 0, 0, 32, 10, 0, 0, 0, 80, 0, 1)
    assert groups_of([100], {"psd_lg_cluster_wgs": 8}) == [one]
    assert groups_of([100, 100], {"psd_lg_cluster_wgs": 8}) == [two]
    assert groups_of([100], {"psd_lg_cluster_wgs": 16}) == [_with(one, cluster=1)]
    assert groups_of([100, 100], {"psd_lg_cluster_wgs": 16}) == [two]
    assert groups_of([100, 100]) == [_with(two, cluster=1)]


def test_forced_64_wide_tiles_switch_the_shrink_and_the_one_launch_kernel_off():
    assert groups_of([270], T64) == [(320, 1, 0, 0, 64, 15, 0, 0, 0, 120, 0, 1)]
    assert groups_of([100, 128], T64) == [(128, 2, 0, 0, 64, 3, 0, 0, 0, 24, 0, 1)]
    assert groups_of([2000], T64) == [(2048, 1, 0, 0, 64, 528, 1, 0, 1, 528, 1, 0)]
    assert groups_of([2000], {"psd_lg_tile": 32, "psd_lg_decide": 1}) == [(2016, 1, 0, 0, 32, 2016, 0, 0, 1, 2016, 1, 0)]


def test_blocks_below_the_sign_path_form_no_group_and_unknown_options_are_refused():
    assert groups_of([64, 8, 33]) == []
    assert groups_of([70, 100], {"psd_sign_min": 101}) == []          # both left to the workgroup eigensolver
    assert groups_of([70, 100, 101], {"psd_sign_min": 101}) == [(128, 1, 0, 0, 32, 10, 0, 1, 0, 80, 0, 1)]
    blk = np.array([100], np.int32)
    keys, vals, _ = H.opt_pairs({"psd_no_such_option": 1})
    out, ng = np.zeros(12, np.int32), C.c_int(0)
    assert lib.cuadmm_psd_sign_groups(P(blk), 1, keys, P(vals), 1, P(out), 1, C.byref(ng)) == -1 and b"psd_no_such_option" in lib.cuadmm_last_error()
    assert lib.cuadmm_psd_sign_groups(P(np.array([100, 200], np.int32)), 2, keys, P(vals), 0, P(out), 1, C.byref(ng)) == -1 and ng.value == 2
