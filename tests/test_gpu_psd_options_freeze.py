"""The projection plan freezes its kernel-selecting options when it is built (csrc/psd_plan.h: PsdRanges): a psd_* option set on
an initialised solver is accepted and logged, and changes nothing in the plan that solver runs.  Before the table, half of these
options were read at every projection while the slots, the rest index, the closed-block records and the partial buffers kept the
layout of init: psd_n32 = 0 or psd_mid = 1 after init ended the next fused solve with "fused projection requested on a plan that
cannot fuse"."""
import numpy as np
import pytest

import cuadmm_amd
from tests import _closed_cases as cc

pytestmark = pytest.mark.gpu


def test_psd_options_set_after_init_leave_the_built_plan_alone():
    # 8 rows on 64 distinct slots per block: 576 one-row trees, so the blocks solve for their own multipliers (closed blocks)
    args = cc.build([24] * 64 + [12] * 8, "dense", 1)

    def run(late_options):
        s = cuadmm_amd.SDPSolver(verbose=False)
        s.init_problem(cuadmm_amd.Problem(*args))
        assert s.counters()["closed_blocks"] == 1
        s.solve(10, 0.0, 0, 50, 100, 0, 1.05)
        for k, v in late_options:
            s.set_option(k, v)
        s.solve(10, 0.0, 0, 50, 100, 0, 1.05, if_first=False)
        assert s.info_iter_num >= 10
        return s.X, s.y, s.S

    ref = run([])
    got = run([("psd_n32", 0), ("psd_w32_occ", 3), ("psd_mid", 1)])
    for a, b in zip(got, ref):
        assert np.all(np.isfinite(b)) and np.array_equal(a, b)
