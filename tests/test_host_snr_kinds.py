"""CPU-only: the planner keys final (fused S/N) launches by S/N kind -- the
row-group form (snr_epilogue) and the segmented form (snr_segments: rows of
240-264 bins, widths <= 9, <= 64 output rows, at least one merge level) run
separate cone_kernel instances -- through rt_schedule_final_kinds, which
builds and validates (validate_exec_plan: no launch of mixed kinds) the plan
rt_plan_create would build.  No device call."""
import ctypes

import numpy as np
import pytest

import inputs

ROWS, SEG = 1, 2                     # bits of bins_kinds[b]
STD_WIDTHS = [1, 2, 3, 4, 6, 9]      # the segmented form's standard ladder
N_TILES = 1 << 17                    # the first rungs take several passes: tile finals


@pytest.fixture(scope="module")
def lib():
    from riptide_amd import _lib
    return _lib.load()


def final_kinds(lib, c, widths):
    """(launches, row-group final launches, segmented final launches,
    {bins: kind bits}) of the plan for case c and these widths."""
    w = np.asarray(widths, dtype=np.uint64)
    u = [ctypes.c_uint64() for _ in range(3)]
    kinds = np.zeros(c["bmax"] + 2, dtype=np.uint8)
    rc = lib.rt_schedule_final_kinds(c["n"], c["tsamp"], w.ctypes.data, w.size, c["pmin"], c["pmax"], c["bmin"],
                                     c["bmax"], *(ctypes.byref(x) for x in u), kinds.ctypes.data, kinds.size)
    assert rc == 0, lib.rt_last_error()
    return u[0].value, u[1].value, u[2].value, {int(b): int(k) for b, k in enumerate(kinds) if k}


@pytest.mark.parametrize("bmin,bmax", [(238, 242), (262, 266)])
def test_final_launches_by_kind_across_the_breakpoints(lib, bmin, bmax):
    """Bins ranges astride 239 | 240 and 264 | 265 (both in the 4- and the
    5-slot bucket's reach: 262-266 is all 5-slot, 238-242 all 4-slot): final
    units of 240-264 bins run in segmented launches only, the others in
    row-group launches only; the split costs at most one launch per final
    launch of the plan built without the segmented form."""
    c = inputs.snr_shape_plan(bmin, bmax, N_TILES)
    launches, nrows, nseg, kinds = final_kinds(lib, c, STD_WIDTHS)
    assert set(range(bmin, bmax + 1)) <= set(kinds)
    for b, k in kinds.items():
        assert k == (SEG if 240 <= b <= 264 else ROWS), (b, k)
    assert nrows >= 1 and nseg >= 1
    # the same plan through rt_schedule_check (no widths: every final unit
    # row-group) has one final launch per (pass, bucket): at most one more each
    u = [ctypes.c_uint64() for _ in range(4)]
    d = [ctypes.c_double() for _ in range(2)]
    assert lib.rt_schedule_check(c["n"], c["tsamp"], len(STD_WIDTHS), c["pmin"], c["pmax"], bmin, bmax,
                                 *(ctypes.byref(x) for x in u[:3]), ctypes.byref(d[0]), ctypes.byref(d[1]),
                                 ctypes.byref(u[3])) == 0, lib.rt_last_error()
    assert u[1].value > u[0].value            # tile finals
    l0, r0, s0, _ = final_kinds(lib, c, [1, 2, 13])
    assert s0 == 0 and nrows + nseg <= 2 * r0


@pytest.mark.parametrize("bmin,bmax", [(238, 242), (262, 266), (257, 266)])
def test_wide_width_or_feature_bit_off_is_row_group(lib, monkeypatch, bmin, bmax):
    """A width list holding 13 (> kSnrSegWmax = 9), or the kConeSnrSeg feature
    bit off (RIPTIDE_AMD_CONE_FLAGS=7), puts every final unit in row-group
    launches."""
    c = inputs.snr_shape_plan(bmin, bmax, N_TILES)
    _, nrows, nseg, kinds = final_kinds(lib, c, STD_WIDTHS + [13])
    assert nseg == 0 and nrows >= 1 and set(kinds.values()) == {ROWS}
    monkeypatch.setenv("RIPTIDE_AMD_CONE_FLAGS", "7")
    try:
        _, nrows, nseg, kinds = final_kinds(lib, c, STD_WIDTHS)
    finally:
        monkeypatch.delenv("RIPTIDE_AMD_CONE_FLAGS")
    assert nseg == 0 and nrows >= 1 and set(kinds.values()) == {ROWS}
    # ... and on again: the segmented launches are back
    assert final_kinds(lib, c, STD_WIDTHS)[2] >= 1


def test_final_unit_over_64_rows_is_row_group(lib):
    """A transform whose final unit holds more than 64 rows is row-group: at
    240 x 70 samples the first rung's 240-242-bin transforms are whole units
    of 69-70 rows (the 4-slot capacity is 72), so their bins have row-group
    final units; at 240 x 60 samples every unit has <= 60 rows and all of
    them are segmented."""
    c = inputs.snr_shape_plan(240, 242, 240 * 70)
    _, nrows, nseg, kinds = final_kinds(lib, c, STD_WIDTHS)
    assert nrows >= 1 and all(kinds[b] & ROWS for b in (240, 241, 242)), kinds
    c = inputs.snr_shape_plan(240, 242, 240 * 60)
    _, nrows, nseg, kinds = final_kinds(lib, c, STD_WIDTHS)
    assert nrows == 0 and nseg >= 1 and set(kinds.values()) == {SEG}, kinds


@pytest.mark.parametrize("scratch,cosched,launches", [("1024", "1", 14), ("1536", None, 8)])
def test_cfg2_bench_schedule_keeps_its_launch_count(lib, monkeypatch, scratch, cosched, launches):
    """The cfg2 bench schedules: 14 launches at 1024 M floats of scratch
    co-scheduled, 8 at 1536 M (one group) -- every final unit segmented, so
    keying final launches by kind splits none."""
    c = inputs.FULL_CASES[1]
    from riptide_amd.ffautils import generate_width_trials
    widths = generate_width_trials(c["bmin"], ducy_max=c["ducy_max"], wtsp=1.5)
    assert max(widths) <= 9
    monkeypatch.setenv("RIPTIDE_AMD_SCRATCH_MFLOATS", scratch)
    if cosched:
        monkeypatch.setenv("RIPTIDE_AMD_COSCHED", cosched)
    try:
        n, nrows, nseg, kinds = final_kinds(lib, c, widths)
    finally:
        monkeypatch.delenv("RIPTIDE_AMD_SCRATCH_MFLOATS")
        if cosched:
            monkeypatch.delenv("RIPTIDE_AMD_COSCHED")
    assert n == launches and nrows == 0 and nseg >= 1
    assert set(kinds) == set(range(240, 261)) and set(kinds.values()) == {SEG}
