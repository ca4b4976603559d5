"""The host-only checks see the plan the device gets: a plan created on the
device reports the launch count rt_schedule_final_kinds reports for the same
parameters and widths, and its ladder is the free ladder_layout's.  Both
sides take their plan from plan_periodogram (riptide_amd/csrc/plan.hpp)."""
import ctypes

import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu

# the reduced cfg2 (240-260 bins, widths <= 9: segmented final launches) and
# cfg3 (the same bins, widths up to 42: past the 12-bin register window)
CASES = [inputs.PGRAM_CASES[1], inputs.PGRAM_CASES[2]]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_created_plan_is_the_checked_plan(case):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from riptide_amd import _lib, engine, generate_width_trials
    w = np.asarray(generate_width_trials(case["bmin"], ducy_max=case["ducy_max"]), dtype=np.uint64)
    assert (w.max() <= 9) if case["name"] == "cfg2" else (w.max() > 12)
    args = (case["n"], case["tsamp"], case["pmin"], case["pmax"], case["bmin"], case["bmax"])
    plan = engine.PeriodogramPlan(args[0], args[1], w, *args[2:])
    launches = ctypes.c_uint64()
    lib = _lib.load()
    rc = lib.rt_schedule_final_kinds(args[0], args[1], w.ctypes.data, w.size, *args[2:], ctypes.byref(launches), None,
                                     None, None, 0)
    assert rc == 0, lib.rt_last_error()
    assert plan.stats()["launches"] == launches.value > 0
    mine, free = plan.ladder_layout(), engine.ladder_layout(*args)
    assert np.array_equal(mine.pop("rungs"), free.pop("rungs")) and mine == free
    assert free["mode"] == 1 and free["leaf_floats"] > 0
