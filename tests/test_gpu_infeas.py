"""Option "infeas_check": certificates of infeasibility from iterate differences ("Infeasibility certificates";
csrc/infeas.hip, csrc/engine_reports.hip: infeas_step).

Op level: the roll kernel against numpy (bit-equal differences, sums against math.fsum).  Engine level: the four infeasible
problems of tests/_infeas_twin.py against the numpy twin under both switch_admm settings; the returned certificates against the
ORIGINAL data with numpy alone; no false alarm and no footprint on a feasible problem and a shipped input; a sequence through an
infeasible step; the refusals; the command line.

Engine against twin.  The engine declares at the twin's check or the next one (the violation falls geometrically and the two may
cross the threshold one period apart); beta / gamma is the limit of a converging ratio and agrees to 1e-6 relative.
Certificate bound: tests/test_infeas_host.py explains the reported radius.
"""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import cuadmm_amd
from tests._infeas_twin import STATUS, make_fixture, twin_solve, verify_dual, verify_primal
from tests.conftest import load_npz_problem
from tests.helpers import problem_to_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
PERIOD, TOL, CAP, STOP = 50, 1e-6, 2000, 1e-6
SGS, ADMM = 11000, 0
INFO = ("pobj", "dobj", "errRp", "errRd", "relgap", "sig")
_twins, _runs = {}, {}


def amd(fx):
    r, c, v = fx.coo()
    bi, ci = np.nonzero(fx.b)[0], np.nonzero(fx.C)[0]
    return cuadmm_amd.Problem.from_coo(fx.blk, fx.m, r, c, v, bi, fx.b[bi], ci, fx.C[ci])


def twin(kind, sw, big):
    key = (kind, sw, big)
    if key not in _twins:
        _twins[key] = twin_solve(make_fixture(kind, big), PERIOD, TOL, CAP, STOP, switch_admm=sw)
    return _twins[key]


def solver(options=None, **kw):
    return cuadmm_amd.SDPSolver(verbose=False, options=options, **kw)


def engine(kind, sw, big, options=None):
    """one solve per (problem, switch), shared by the tests that read it"""
    key = (kind, sw, big)
    if key not in _runs or options is not None:
        s = solver(dict({"infeas_check": PERIOD, "infeas_tol": TOL}, **(options or {})))
        s.init_problem(amd(make_fixture(kind, big)))
        s.solve(CAP, STOP, 500, 50, 100, sw, 1.05)
        if options is not None:
            return s
        _runs[key] = s
    return _runs[key]


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------
SPAN = 512          # doubles one workgroup covers per pass on the 16-byte path (256 threads x 2); 256 on the one-double path


def _roll(cur, prev, w, negate=0, ranges=(), offset=0):
    lib = cuadmm_amd.load()
    n = cur.size
    prev = prev.copy()
    d, sums = np.full(n, np.nan), np.zeros(2)
    zo = np.array([r[0] for r in ranges], np.int64)
    zl = np.array([r[1] for r in ranges], np.int64)
    rc = lib.cuadmm_op_infeas_roll(n, P(cur), P(prev), P(w), negate, len(ranges), P(zo) if len(ranges) else None, P(zl) if len(ranges) else None,
                                   offset, P(d), P(sums))
    assert rc == 0, lib.cuadmm_last_error()
    return prev, d, sums


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 255, 256, 257, 3 * SPAN + 5, 1024 * SPAN + 3 * SPAN + 5])
def test_roll_kernel(n, offset):
    """the last length wraps the fixed stride of 1 024 workgroups: every thread takes a second item"""
    rng = np.random.default_rng(n + offset)
    cur, prev, w = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    ref = cur - prev
    p1, d1, s1 = _roll(cur, prev, w, offset=offset)
    assert np.array_equal(p1, cur) and np.array_equal(d1, ref)
    # math.fsum adds numpy's products exactly; those are rounded once each, while the kernel's multiply-adds may be fused: a
    # difference of a few eps sqrt(n) times the products' magnitude, far inside the bound for these seeds
    for got, a, b in ((s1[0], ref, ref), (s1[1], w, ref)):
        want = math.fsum(a * b)
        print("n %d offset %d: sum %.17g, reference %.17g, rel %.2e" % (n, offset, got, want, abs(got - want) / abs(want)))
        assert abs(got - want) <= 1e-13 * abs(want)
    _, _, s2 = _roll(cur, prev, w, offset=offset)
    assert np.array_equal(s1, s2)                                   # bit-identical from run to run
    ranges = [(0, 1)] if n < 7 else [(1, 3), (n - 2, 2)] + ([(300, 700)] if n > 1100 else [])
    p3, d3, s3 = _roll(cur, prev, w, negate=1, ranges=ranges, offset=offset)
    want = -ref
    for lo, ln in ranges:
        want[lo:lo + ln] = 0.0
    assert np.array_equal(d3, want) and np.array_equal(p3, cur)
    assert np.array_equal(s3, s1)                                   # the sums are those of the plain difference


# ---- 2. P, D, P3, D3 with the engine against the twin ---------------------------------------------------------------------
CASES = [(k, sw, big) for k in "PD" for big in (False, True) for sw in (SGS, ADMM)]


@pytest.mark.parametrize("kind,sw,big", CASES)
def test_verdict_against_the_twin(kind, sw, big):
    t, s = twin(kind, sw, big), engine(kind, sw, big)
    st = s.status()
    print("%s%s switch %d: engine %s at %d (twin at %d), scalar %.9g (twin %.9g), eta %.3g, radius %.4g, checks %d, %.2f ms, %.0f bytes"
          % (kind, "3" if big else "", sw, st["name"], st["iteration"], t.iteration, st["scalar"], t.scalar, st["eta"], st["radius"], st["checks"], st["ms"], st["bytes"]))
    assert t.status == (3 if kind == "P" else 4)
    assert st["status"] == t.status and st["name"] == STATUS[t.status]
    assert st["iteration"] in (t.iteration, t.iteration + PERIOD)
    assert abs(st["scalar"] - t.scalar) <= 1e-6 * abs(t.scalar)
    assert st["eta"] <= TOL * st["scalar"] and st["checks"] == st["iteration"] // PERIOD - 1
    assert s.info_iter_num == st["iteration"] and st["bytes"] > 0


@pytest.mark.parametrize("kind,sw,big", CASES)
def test_certificate_against_the_original_data(kind, sw, big):
    fx, s = make_fixture(kind, big), engine(kind, sw, big)
    which, ray = s.certificate()
    R = s.status()["radius"]
    assert np.isfinite(R) and R > 0
    if kind == "P":
        assert which == "primal" and ray.shape == (fx.m,)
        e, v = verify_primal(fx, ray, R)
    else:
        assert which == "dual" and ray.shape == (fx.L,)
        e, v = verify_dual(fx, ray, R)
    print("%s%s switch %d: normalisation error %.2e, violation x radius %.12f" % (kind, "3" if big else "", sw, e, v))
    assert abs(e) <= 1e-12
    assert v <= 1 + 1e-9


# ---- 3. no false alarm, no footprint --------------------------------------------------------------------------------------
def _traj(s):
    return [s.info_arr(k).copy() for k in INFO] + [s.X, s.y, s.S]


SHIPPED = (100000, 1e-3, 500, 50, 100)      # the shipped inputs to convergence at 1e-3 (NOTEBOOK.md: 202 and 139 iterations)


@pytest.mark.parametrize("name,sw", [("F", SGS), ("F", ADMM), ("F3", SGS), ("PlanarHand_N=1_MOMENT", SGS), ("PlanarHand_N=1_MOMENT", ADMM),
                                     ("taha1a", SGS)])
def test_no_false_alarm_no_footprint(name, sw):
    """every run ends converged; with the check on (period 25) it is the same run bit for bit"""
    fixture = name.startswith("F")
    p = amd(make_fixture("F", name == "F3")) if fixture else problem_to_amd(load_npz_problem(name))
    args = (CAP, STOP, 500, 50, 100) if fixture else SHIPPED
    runs = []
    for opts in (None, {"infeas_check": 25}):
        s = solver(opts)
        s.init_problem(p)
        s.solve(*args, sw, 1.05)
        runs.append(s)
    off, on = runs
    for a, b in zip(_traj(off), _traj(on)):
        assert np.array_equal(a, b)
    st = on.status()
    print(name, sw, st)
    assert st["status"] == 1 and st["name"] == "converged" and st["checks"] > 0
    assert off.status()["status"] == 1 and off.status()["checks"] == 0 and off.status()["iteration"] == st["iteration"]
    with pytest.raises(RuntimeError):
        on.certificate()


# ---- 4. a sequence through an infeasible step -----------------------------------------------------------------------------
@pytest.mark.parametrize("sw", [SGS, ADMM])
def test_sequence_through_an_infeasible_step(sw):
    fF, fP = make_fixture("F"), make_fixture("P")
    bi = np.arange(fF.m, dtype=np.int32)
    args = (CAP, STOP, 500, 50, 100, sw, 1.05)
    s = solver({"infeas_check": PERIOD})
    s.init_problem(amd(fF))
    s.solve(*args)
    assert s.status()["status"] == 1
    s.update_bC(bi, fP.b, None, None, False, 1.0)
    assert s.status()["status"] == 0
    s.solve(*args)
    assert s.status()["name"] == "primal_infeasible"
    e, v = verify_primal(fP, s.certificate()[1], s.status()["radius"])
    assert abs(e) <= 1e-12 and v <= 1 + 1e-9
    s.update_bC(bi, fF.b, None, None, False, 1.0)
    s.solve(*args)
    assert s.status()["status"] == 1
    # a solver that never saw the infeasible step
    q = solver({"infeas_check": PERIOD})
    q.init_problem(amd(fF))
    q.solve(*args)
    q.update_bC(bi, fF.b, None, None, False, 1.0)
    q.solve(*args)
    for a, b in zip(_traj(s), _traj(q)):
        assert np.array_equal(a, b)
    # the same three steps with the option off (the infeasible one runs to the iteration limit): nothing of the check -- its
    # snapshots, its status, its second plan -- reaches the solve behind the next update_bC
    r = solver()
    r.init_problem(amd(fF))
    r.solve(*args)
    r.update_bC(bi, fP.b, None, None, False, 1.0)
    r.solve(*args)
    assert r.status()["name"] == "iteration_limit"
    r.update_bC(bi, fF.b, None, None, False, 1.0)
    r.solve(*args)
    assert r.status()["status"] == 1 and r.status()["checks"] == 0
    for a, b in zip(_traj(s), _traj(r)):
        assert np.array_equal(a, b)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    p = amd(make_fixture("F"))
    for opts, kw in (({"infeas_check": 50, "accel": 4}, {}), ({"infeas_check": 50}, {"world": 2}), ({"infeas_check": 50}, {"eig_rank": 2})):
        s = solver(opts, **kw)
        with pytest.raises(RuntimeError, match="infeas_check"):
            s.init_problem(p)
    with pytest.raises(RuntimeError, match="infeas_check"):
        solver({"infeas_check": 1})
    s = solver({"infeas_check": 50})
    s.init_problem(p)
    with pytest.raises(RuntimeError, match="infeas_check"):
        s.set_option("infeas_check", 25)                            # the period is set before init
    lib, got = cuadmm_amd.load(), C.c_double()
    for key in (b"infeas_check", b"gap_check"):                     # the two keys refused on an initialised solver, in their words
        assert lib.cuadmm_set_option(s._h, key, C.c_double(25)) == -1 and lib.cuadmm_last_error() == b"set_option: %s is set before init" % key
        assert lib.cuadmm_set_option(s._h, key, C.c_double(1)) == -1                              # (the range is checked first, as it was)
        assert lib.cuadmm_last_error() == b"set_option: %s must be 0 (off) or an integer period from 2 to 1000000" % key
        assert lib.cuadmm_get_option(s._h, key, C.byref(got)) == 0 and got.value == (50 if key == b"infeas_check" else 0)
    assert lib.cuadmm_set_option(s._h, b"infeas_tol", C.c_double(1e-6)) == 0                      # (its default) every other key stays settable
    s.solve(CAP, STOP, 500, 50, 100, SGS, 1.05)
    assert s.status()["status"] == 1
    with pytest.raises(RuntimeError, match="certificate"):
        s.certificate()


# ---- 6. command line ------------------------------------------------------------------------------------------------------
def _write_dir(d, fx):
    os.makedirs(d)
    with open(d + "blk.txt", "w") as f:
        f.write("".join("%s %d\n" % ("s" if n > 0 else "u", abs(n)) for n in fx.blk))
    with open(d + "con_num.txt", "w") as f:
        f.write("%d\n" % fx.m)
    r, c, v = fx.coo()
    with open(d + "At.txt", "w") as f:
        for i, j, x in zip(r, c, v):
            f.write("%d %d %.17g\n" % (int(i), int(j), float(x)))
    for nm, vec in (("b.txt", fx.b), ("C.txt", fx.C)):
        with open(d + nm, "w") as f:
            for i in np.nonzero(vec)[0]:
                f.write("%d 0 %.17g\n" % (int(i), float(vec[i])))


def test_cli_status(tmp_path):
    dP, dF = str(tmp_path / "dirP") + "/", str(tmp_path / "dirF") + "/"
    _write_dir(dP, make_fixture("P"))
    os.makedirs(dF)
    fF = make_fixture("F")
    with open(dF + "b.txt", "w") as f:
        for i in np.nonzero(fF.b)[0]:
            f.write("%d 0 %.17g\n" % (int(i), float(fF.b[i])))
    exe = os.path.join(ROOT, "cuadmm_amd", "lib", "cuadmm_exe")
    js = str(tmp_path / "run.json")
    r = subprocess.run([exe, dP, "--then=" + dF, "--infeas=50", "--max_iter=2000", "--stop_tol=1e-6", "--json=" + js], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Solver ended: primal infeasible (certificate at iteration" in r.stdout
    with open(js) as f:
        side = json.load(f)
    assert side["status"] == "primal_infeasible" and side["infeas"]["checks"] >= 1
    with open(js + ".1") as f:                                      # the infeasible stage did not stop the sequence
        assert json.load(f)["status"] == "converged"
