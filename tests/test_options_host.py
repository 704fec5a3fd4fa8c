"""The option tables (csrc/option_table.h, csrc/psd_options.h) against expectations written out by hand from the chain of comparisons that
cuadmm_set_option and PsdOptions::set were before them: what each key stores, what it refuses and in which words, the defaults and the
environment variables behind them, and the two documents that list the keys.  A fresh handle touches no device."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest

import cuadmm_amd
from tests.conftest import ROOT

lib = cuadmm_amd.load()

RETIRED = ("psd_lg_clean", "psd_graph", "tail_prefetch", "tail_depth", "tail_order", "tail_rb", "tail_zreg", "tail_group_pf", "tail_fat", "tail_dd",
           "tail_pinv_tol", "pinv_tol", "lead_tops_refine", "graph")
REAL_KEYS = {"eig_rank_maxfeas", "batch_mixed", "accel_safeguard", "accel_reg", "infeas_tol", "gap_tol"}
# keys with a rule and a message of their own, which answers before the two general refusals do
OWN_RULE = {"accel": b"set_option: accel must be an integer from 0 (off) to 16",
            "infeas_check": b"set_option: infeas_check must be 0 (off) or an integer period from 2 to 1000000",
            "infeas_tol": b"set_option: infeas_tol must not be negative",
            "gap_check": b"set_option: gap_check must be 0 (off) or an integer period from 2 to 1000000",
            "gap_tol": b"set_option: gap_tol must not be negative"}


def table():
    rows = []
    for i in range(lib.cuadmm_option_count()):
        key, env, default, flags = C.c_char_p(), C.c_char_p(), C.c_double(), C.c_uint()
        assert lib.cuadmm_option_info(i, C.byref(key), C.byref(env), C.byref(default), C.byref(flags)) == 0
        rows.append((key.value.decode(), env.value.decode() if env.value else None, default.value, flags.value))
    return rows


@pytest.fixture()
def handle():
    h = C.c_void_p()
    assert lib.cuadmm_create(C.byref(h)) == 0
    yield h
    lib.cuadmm_destroy(h)


def set_opt(h, key, value):
    return lib.cuadmm_set_option(h, key.encode(), C.c_double(value))


def get_opt(h, key):
    v = C.c_double(math.nan)
    assert lib.cuadmm_get_option(h, key.encode(), C.byref(v)) == 0, key
    return v.value


def test_table_keys_are_unique_and_every_key_takes_and_holds_its_default(handle):
    rows = table()
    keys = [r[0] for r in rows]
    envs = [r[1] for r in rows if r[1]]
    assert len(rows) == 69 and len(set(keys)) == len(keys) and len(set(envs)) == len(envs)
    assert lib.cuadmm_option_info(len(rows), None, None, None, None) != 0 and lib.cuadmm_option_info(-1, None, None, None, None) != 0
    for key, env, default, flags in rows:
        assert get_opt(handle, key) == default, key                     # the struct's initialiser and the table agree
        assert set_opt(handle, key, default) == 0 and get_opt(handle, key) == default, key
        assert (flags & 3 == 2) == (key in REAL_KEYS), key
        assert bool(flags & 256) == (key.startswith("psd_") and key not in ("psd_steps", "psd_hint")), key      # (those two are the engine's)
    # a few rows against the parent's code, column by column: (env, default, flags = kind | when << 2 | group << 4 | negated << 6 | eig/lds << 7 | psd << 8)
    by_key = {r[0]: r[1:] for r in rows}
    assert by_key["device"] == (None, 0.0, 0 | 1 << 2 | 1 << 4)
    assert by_key["mapped_out"] == ("CUADMM_NO_MAPPED_OUT", 1.0, 0 | 1 << 2 | 64)
    assert by_key["infeas_check"] == (None, 0.0, 0)
    assert by_key["accel_reg"] == (None, 1e-10, 2 | 3 << 2)
    assert by_key["duo_inject_fail"] == (None, 0.0, 1 | 3 << 2 | 2 << 4)
    assert by_key["psd_mid"] == ("CUADMM_PSD_MID", 0.0, 0 | 2 << 2 | 128 | 256)
    assert by_key["psd_overlap"] == ("CUADMM_PSD_OVERLAP", 1.0, 0 | 3 << 2 | 256)
    assert by_key["tail_max_k"][1] == 32768 and by_key["batch"][1] == 64 and by_key["psd_sign_ws_mb"][1] == 8192 and by_key["fuse_solve"][1] == -1
    assert sorted(k for k, r in by_key.items() if (r[2] >> 4) & 3 == 1) == ["device", "rank", "verbose", "world"]      # what a group does not share
    assert sorted(e for e in envs if not e.startswith("CUADMM_PSD_") or e == "CUADMM_PSD_HINT") == [
        "CUADMM_FUSE", "CUADMM_FUSE_ROWS", "CUADMM_FUSE_SOLVE", "CUADMM_HOST_SCALARS", "CUADMM_HOST_SOLVE", "CUADMM_NO_LOCAL_CONSTRAINTS",
        "CUADMM_NO_MAPPED_OUT", "CUADMM_PSD_HINT", "CUADMM_TAIL_K"]


@pytest.mark.parametrize("key,value,stored", [
    ("batch", 300, 256), ("batch", -5, 0), ("batch", 2.9, 2),
    ("psd_w32_occ", 5, 4), ("psd_w32_occ", 3, 3), ("psd_cu_occ", 3, 3), ("psd_cu_occ", 0, 4),
    ("psd_sign_min", 10, 65), ("psd_sign_min", 200, 200), ("psd_lg_cluster_wgs", 5, 8), ("psd_lg_cluster_wgs", 2000, 960),
    ("psd_sign_ws_mb", 0, 1), ("psd_debug", -1, 0), ("tail_k", -1.5, -1), ("lead_small_kb", 99, 99), ("batch_mixed", 7, 1), ("batch_mixed", 0.25, 1),
    ("accel_safeguard", -1.0, -1.0),
    ("lpt", 0, 0), ("eig_rank_maxfeas", 1e-3, 1e-3), ("psd_wave4_min", 17.5, 17), ("infeas_tol", 1e300, 1e300), ("duo_inject_fail", 4e12, 4e12),
    ("accel", 16, 16), ("infeas_check", 2, 2), ("gap_check", 1000000, 1000000), ("gap_tol", 0, 0), ("fuse_solve", -7.9, -7),
])
def test_stored_value(handle, key, value, stored):
    assert set_opt(handle, key, value) == 0, lib.cuadmm_last_error()
    assert get_opt(handle, key) == stored


@pytest.mark.parametrize("key,value", [("accel", 17), ("accel", -1), ("accel", 2.5), ("accel", math.nan), ("infeas_check", 1), ("infeas_check", 1000001),
                                       ("infeas_check", 2.5), ("infeas_tol", -1e-12), ("infeas_tol", math.nan), ("gap_check", 1), ("gap_check", -3),
                                       ("gap_tol", -1.0), ("gap_tol", math.nan)])
def test_refusals_of_the_keys_with_a_rule_keep_their_words_and_leave_the_value(handle, key, value):
    before = get_opt(handle, key)
    assert set_opt(handle, key, value) == -1
    assert lib.cuadmm_last_error() == OWN_RULE[key]
    assert get_opt(handle, key) == before


def test_unknown_retired_and_null_keys(handle):
    for key in ("no_such_option",) + RETIRED:
        assert set_opt(handle, key, 1) == -1
        assert lib.cuadmm_last_error() == b"set_option: unknown key '%s'" % key.encode()
        v = C.c_double()
        assert lib.cuadmm_get_option(handle, key.encode(), C.byref(v)) == -1
    assert lib.cuadmm_set_option(handle, None, C.c_double(1)) == -1 and lib.cuadmm_last_error() == b"set_option: null"
    assert lib.cuadmm_set_option(None, b"fuse", C.c_double(1)) == -1 and lib.cuadmm_last_error() == b"set_option: null"


def test_no_key_takes_a_value_that_is_not_finite_and_no_integer_key_one_beyond_int(handle):
    """NaN and the infinities are refused by every key; +-1e300 by every key that stores an integer.  The six real keys keep taking any finite
    value their own rule admits, as they did (batch_mixed: non-zero is true): 1e300 is a value of a double."""
    for key, env, default, flags in table():
        for bad in (math.nan, math.inf, -math.inf, 1e300, -1e300):
            rc = set_opt(handle, key, bad)
            msg = lib.cuadmm_last_error() if rc else None
            if math.isfinite(bad) and key in REAL_KEYS:
                if key in OWN_RULE and bad < 0:
                    assert rc == -1 and msg == OWN_RULE[key]
                else:
                    assert rc == 0 and get_opt(handle, key) == (bad if key != "batch_mixed" else 1.0)
                    assert set_opt(handle, key, default) == 0
                continue
            assert rc == -1, (key, bad)
            if key in OWN_RULE and (key not in REAL_KEYS or not bad > 0):        # (+inf is not negative: infeas_tol and gap_tol get the general answer)
                assert msg == OWN_RULE[key], (key, bad)
            else:
                want = b"set_option: %s takes a finite value" if not math.isfinite(bad) else b"set_option: %s is out of range"
                assert msg == want % key.encode(), (key, bad)
            assert get_opt(handle, key) == default, (key, bad)
    for bad, rc in ((2147483647.9, 0), (2147483648.0, -1), (-2147483648.9, 0), (-2147483649.0, -1)):
        assert set_opt(handle, "tail_k", bad) == rc, bad
    assert get_opt(handle, "tail_k") == -2147483648.0


_CHILD = """
import ctypes as C, sys
import cuadmm_amd
lib = cuadmm_amd.load()
h = C.c_void_p()
assert lib.cuadmm_create(C.byref(h)) == 0
for key in sys.argv[1:]:
    v = C.c_double()
    assert lib.cuadmm_get_option(h, key.encode(), C.byref(v)) == 0
    print(key, v.value)
lib.cuadmm_destroy(h)
"""
_ENV_KEYS = ("fuse", "mapped_out", "local_constraints", "tail_k", "psd_hint", "psd_mid", "psd_n16", "psd_lg_cluster_wgs")


def _child_defaults(extra_env):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CUADMM_")}
    env.update(extra_env)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", _CHILD] + list(_ENV_KEYS), env=env, cwd=ROOT, check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[0]: float(line.split()[1]) for line in out.splitlines()}


def test_environment_gives_the_defaults_of_a_new_handle():
    got = _child_defaults({"CUADMM_FUSE": "0", "CUADMM_NO_MAPPED_OUT": "1", "CUADMM_NO_LOCAL_CONSTRAINTS": "1", "CUADMM_TAIL_K": "512", "CUADMM_PSD_HINT": "3",
                           "CUADMM_PSD_MID": "lds", "CUADMM_PSD_N16": "eig", "CUADMM_PSD_LG_CLUSTER_WGS": "5000"})
    assert got == {"fuse": 0, "mapped_out": 0, "local_constraints": 0, "tail_k": 512, "psd_hint": 3, "psd_mid": 2, "psd_n16": 0, "psd_lg_cluster_wgs": 960}


def test_without_the_environment_a_new_handle_has_the_built_in_defaults():
    got = _child_defaults({})
    assert got == {"fuse": 1, "mapped_out": 1, "local_constraints": 1, "tail_k": -1, "psd_hint": 1, "psd_mid": 0, "psd_n16": 1, "psd_lg_cluster_wgs": 224}


def test_the_two_documents_list_the_keys_of_the_tables_and_no_others():
    keys = [r[0] for r in table()]
    integ = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    sec6 = integ[integ.index("\n## 6. Engine options"):integ.index("\n## 7. ")]
    hdr = open(os.path.join(ROOT, "include", "cuadmm_amd.h"), encoding="utf-8").read()
    block = hdr[hdr.index("/* Engine options; call before cuadmm_init."):hdr.index("int cuadmm_set_option(")]
    rows6 = [line for line in sec6.splitlines() if line.startswith("| `")]
    listed = [k for line in rows6 for k in re.findall(r"`([a-z][a-zA-Z0-9_]*)`", line.split("|")[1])]
    assert listed == keys                                               # section 6: every key once, in table order
    quoted = re.findall(r'"([a-z][a-zA-Z0-9_]*)"', block)               # (the titles of DESIGN.md's sections are quoted too: capitals, spaces)
    assert quoted and all(k in keys for k in quoted)
    assert [k for k in keys if k in quoted] == list(dict.fromkeys(quoted))      # the header's block: table order
    for k in re.findall(r"`([a-z][a-z0-9_]*)`", sec6[:sec6.index("\n| option (default)")]):      # the prose above the table names retired keys only as such
        assert k in keys or k in RETIRED or k.startswith("cuadmm_"), k
    defaults = {r[0]: r[2] for r in table()}
    for line in rows6:                                                  # `key` (default) in the first column: the table's default
        for k, d in re.findall(r"`([a-zA-Z0-9_]+)` \(([-−0-9.e ]+)\)", line.split("|")[1]):
            assert float(d.replace("−", "-").replace(" ", "")) == defaults[k], k


def test_the_plan_hooks_tell_an_unknown_key_from_a_refused_value():
    """cuadmm_psd_sign_groups (host only) takes its options through PsdOptions::set: the message for an unknown key is the old one, and a
    known key with a value no key takes is not called unknown."""
    import numpy as np
    blk, out, ng = np.array([100], np.int32), np.zeros(12, np.int32), C.c_int()
    for key, value, msg in ((b"psd_no_such_option", 1.0, b"psd_sign_groups: unknown option psd_no_such_option"),
                            (b"psd_lg_tile", math.nan, b"psd_sign_groups: option psd_lg_tile takes a finite value"),
                            (b"psd_lg_tile", 1e300, b"psd_sign_groups: option psd_lg_tile is out of range")):
        keys, vals = (C.c_char_p * 1)(key), np.array([value])
        rc = lib.cuadmm_psd_sign_groups(blk.ctypes.data_as(C.c_void_p), 1, keys, vals.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p), 1, C.byref(ng))
        assert rc == -1 and lib.cuadmm_last_error() == msg


def test_the_tables_run_clean_under_the_host_sanitizers():
    """tests/option_table_selftest.cpp, a program of its own (no library; the sanitizers' runtimes linked into it, so no preload): every row of
    both tables through store and get, the stored values above and the refused ones, under ASan + UBSan.  Built once (cuadmm_amd.build)."""
    from cuadmm_amd import build as b
    exe = b.build_option_selftest()
    env = {k: v for k, v in os.environ.items() if not k.startswith("CUADMM_")}
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "69 keys, 0 failures" in r.stdout, r.stdout
