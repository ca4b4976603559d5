"""CPU-only tests of the single-pulse search: the host specification
(rt_single_pulse_host, pulse_host.hpp) against the numpy restatement of
pulse_common, its tie and edge rules and error returns, the width ladder, the
clustering of events into pulses, and the sanitizer build of the checker."""
import os
import subprocess

import numpy as np
import pytest

import pulse_common as pc
from conftest import REPO, snr_close


@pytest.fixture(scope="module")
def sp():
    from riptide_amd import single_pulse
    return single_pulse


PULSES = [(0, 10, 1, 3.5), (1, 30, 7, 1.5), (0, 1000, 40, 0.75), (2, 1020, 3, 2.0), (1, 4090, 12, 1.25),
          (0, 4099 - 5, 5, 2.0), (1, 12000, 64, 0.5), (0, -2, 6, 2.0)]


@pytest.mark.parametrize("B,N", [(1, 64), (3, 4099), (2, 20000)])
@pytest.mark.parametrize("R", [1, 64, 5000])
def test_dyadic_rows_are_bit_identical(sp, B, N, R):
    """On dyadic inputs every float64 sum is exact in any order: best, kbest
    and the events equal the restatement bit for bit, at thresholds that give
    none, a few and thousands of events."""
    widths = sp.generate_pulse_widths(64)
    x = pc.dyadic_rows(100 + N, B, N, PULSES)
    ev, best, kbest = sp.single_pulse_host(x, widths, 1000.0, radius=R, dense=True)
    _, rbest, rkbest = pc.numpy_single_pulse(x, widths, 1000.0, R)
    assert ev.size == 0
    assert np.array_equal(best.view(np.uint32), rbest.view(np.uint32))
    assert np.array_equal(kbest, rkbest)
    counts = []
    for thr in (3.0, -100.0 if R == 1 else 2.0):
        ev = sp.single_pulse_host(x, widths, thr, radius=R)
        ref = pc.numpy_single_pulse(x, widths, thr, R)[0]
        assert pc.events_equal(ev, ref), (thr, ev.size, ref.size)
        assert np.all(np.diff(ev["series"].astype(np.int64) * N + ev["sample"]) > 0)
        counts.append(ev.size)
    assert counts[0] > 0
    if R == 1 and N >= 4099:
        assert counts[1] > 1000


def test_row_stride(sp):
    """ldx = N + 5: the rows of a wider array are read in place."""
    widths = sp.generate_pulse_widths(64)
    N = 4099
    wide = np.full((3, N + 5), np.nan, dtype=np.float32)
    wide[:, :N] = pc.dyadic_rows(7, 3, N, PULSES)
    view = wide[:, :N]
    assert view.strides[0] == 4 * (N + 5)
    got = sp.single_pulse_host(view, widths, 4.0, radius=64, dense=True)
    ref = sp.single_pulse_host(np.ascontiguousarray(view), widths, 4.0, radius=64, dense=True)
    assert pc.events_equal(got[0], ref[0]) and got[0].size > 0
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert pc.events_equal(got[0], pc.numpy_single_pulse(view, widths, 4.0, 64)[0])


@pytest.mark.parametrize("B,N", [(1, 64), (3, 4099), (2, 20000)])
def test_gaussian_rows_within_snr_tolerance(sp, B, N):
    """Seeded float32 noise: the pinned summation order differs from a
    sequential cumsum by rounding only."""
    widths = sp.generate_pulse_widths(64)
    x = pc.gaussian_rows(N, B, N, PULSES)
    _, best, _ = sp.single_pulse_host(x, widths, 8.0, dense=True)
    _, rbest, _ = pc.numpy_single_pulse(x, widths, 8.0, 64)
    ok, msg = snr_close(best, rbest)
    assert ok, msg


def test_long_windows_cross_segments(sp):
    """Widths above the 1024-sample restart of the partial sums: a window
    holds whole segments."""
    widths = np.array([1, 1000, 1024, 1025, 3000, 6144], dtype=np.int32)
    x = pc.dyadic_rows(5, 2, 9000, [(0, 2000, 3000, 0.25), (1, 100, 1024, 0.5)])
    got = sp.single_pulse_host(x, widths, 6.0, radius=6144, dense=True)
    ref = pc.numpy_single_pulse(x, widths, 6.0, 6144)
    assert pc.events_equal(got[0], ref[0]) and got[0].size > 0
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)) and np.array_equal(got[2], ref[2])


def test_plateau_and_width_ties(sp):
    """Equal neighbours give one event, at the leftmost sample; equal S/N at
    two widths gives the smaller width."""
    x = np.zeros(40, dtype=np.float32)
    x[10:14] = 3.0                       # width 1: a plateau of four equal samples
    ev, best, kbest = sp.single_pulse_host(x, [1], 2.0, radius=5, dense=True)
    assert ev["sample"].tolist() == [10] and ev["snr"].tolist() == [3.0] and ev["iwidth"].tolist() == [0]
    assert best[0, 10:14].tolist() == [3.0] * 4
    # widths 1 and 4: sample 2 alone gives 2 / sqrt(1) = 2, the window [0, 4) gives 4 / sqrt(4) = 2
    y = np.zeros(12, dtype=np.float32)
    y[0:4] = [0.5, 0.5, 2.0, 1.0]
    ev, best, kbest = sp.single_pulse_host(y, [1, 4], 1.5, radius=12, dense=True)
    assert best[0, 2] == 2.0 and kbest[0, 2] == 0
    assert ev["sample"].tolist() == [2] and ev["iwidth"].tolist() == [0]
    # a NaN never wins and never becomes an event (it spoils the partial sums
    # of the rest of its 1024-sample segment, as it would a prefix sum)
    z = np.zeros(16, dtype=np.float32)
    z[2] = 4.0
    z[9] = np.nan
    ev, best, kbest = sp.single_pulse_host(z, [1, 2], 1.0, radius=3, dense=True)
    assert not np.any(np.isnan(best)) and best[0, 9] == -np.inf and kbest[0, 9] == -1
    assert ev["sample"].tolist() == [2]


def test_edge_rule(sp):
    """Widths that do not fit at t are skipped: at the ends only the narrow
    widths count, and a width that fits nowhere around t leaves -inf."""
    x = np.ones(10, dtype=np.float32)
    _, best, kbest = sp.single_pulse_host(x, [4, 10], 100.0, dense=True)
    # width 4 (c = 2) fits for 2 <= t <= 8, width 10 (c = 5) at t = 5 alone
    assert kbest.tolist() == [[-1, -1, 0, 0, 0, 1, 0, 0, 0, -1]]
    assert np.all(best[0, [0, 1, 9]] == -np.inf)
    assert best[0, 2] == 2.0 and best[0, 5] == np.float32(10.0 / np.sqrt(10.0))
    ref = pc.numpy_single_pulse(x, [4, 10], 100.0, 10)
    assert np.array_equal(best, ref[1]) and np.array_equal(kbest, ref[2])


def test_errors(sp):
    from riptide_amd import engine
    x = np.zeros((2, 100), dtype=np.float32)
    big = np.zeros(engine.PULSE_MAX_WIDTH + 10, dtype=np.float32)
    assert engine.PULSE_MAX_WIDTH >= 1024
    with pytest.raises(ValueError, match="no trial widths"):
        sp.single_pulse_host(x, [], 8.0)
    with pytest.raises(ValueError, match=">= 1"):
        sp.single_pulse_host(x, [0, 2], 8.0)
    with pytest.raises(ValueError, match="strictly ascending"):
        sp.single_pulse_host(x, [1, 3, 3], 8.0)
    with pytest.raises(ValueError, match="strictly ascending"):
        sp.single_pulse_host(x, [4, 2], 8.0)
    with pytest.raises(ValueError, match="exceeds the series"):
        sp.single_pulse_host(x, [1, 101], 8.0)
    with pytest.raises(ValueError, match="RT_PULSE_MAX_WIDTH"):
        sp.single_pulse_host(big, [1, engine.PULSE_MAX_WIDTH + 1], 8.0, radius=4)
    with pytest.raises(ValueError, match="radius above RT_PULSE_MAX_WIDTH"):
        sp.single_pulse_host(x, [1, 2], 8.0, radius=engine.PULSE_MAX_WIDTH + 1)
    for thr in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match="finite"):
            sp.single_pulse_host(x, [1, 2], thr)
    # the limits themselves pass
    ev = sp.single_pulse_host(big, [1, engine.PULSE_MAX_WIDTH], 8.0, radius=engine.PULSE_MAX_WIDTH)
    assert ev.size == 0


PLAN_WMAX = (1, 7, 64, 1023, 1024, 1025, 2048, 3000, 4096, 5000, 6144)
PLAN_RADIUS = (0, 1, 64, 512, 1024, 2048, 3000, 4096, 5000, 6144)


def test_plan_table(sp):
    """engine.pulse_plan (rt_single_pulse_plan, the device form's planner)
    over a table of (largest width, radius): the tile fits the 160 KiB of
    LDS, the chunk is the whole T + 2R rounded up to segments or the largest
    multiple of 1024 that fits by the header's own formula, and a full tile
    takes 1, 2, 3, 4 or 6 chunks: the classes test_gpu_pulse_paths.py runs."""
    from riptide_amd import engine
    T, lds_max, seg_bytes = engine.PULSE_TILE, 160 << 10, 8 * 1088
    classes = set()
    for wmax in PLAN_WMAX:
        for R in PLAN_RADIUS:
            chunk, segs, lds = engine.pulse_plan(wmax, R)
            what = (wmax, R, chunk, segs, lds)
            fixed = 4 * (T + 2 * R) + 2 * T + 320
            assert lds <= lds_max, what
            assert chunk > 0 and chunk % 1024 == 0, what
            assert segs == (chunk + wmax + 2045) // 1024, what
            assert lds == fixed + seg_bytes * segs, what
            whole = -(-(T + 2 * R) // 1024) * 1024
            more = fixed + seg_bytes * ((chunk + 1024 + wmax + 2045) // 1024)
            assert chunk == whole or (chunk < whole and more > lds_max), what
            classes.add(-(-(T + 2 * R) // chunk))
    assert classes == {1, 2, 3, 4, 6}
    # the plan nearest the limit, and the limits themselves
    assert engine.pulse_plan(5000, 2048) == (8192, 14, 163136)
    assert engine.pulse_plan(6144, 6144) == (3072, 10, 161088)
    for bad in ((0, 4), (engine.PULSE_MAX_WIDTH + 1, 4), (64, engine.PULSE_MAX_WIDTH + 1), (-1, 4), (64, -1)):
        with pytest.raises(ValueError):
            engine.pulse_plan(*bad)


def test_generate_pulse_widths(sp):
    assert sp.generate_pulse_widths(1).tolist() == [1]
    assert sp.generate_pulse_widths(64).tolist() == [1, 2, 3, 4, 6, 9, 13, 19, 28, 42, 63]
    assert sp.generate_pulse_widths(512).tolist()[-4:] == [141, 211, 316, 474]
    assert sp.generate_pulse_widths(20, factor=2.0).tolist() == [1, 2, 4, 8, 16]
    w = sp.generate_pulse_widths(6144)
    assert w.dtype == np.int32 and np.all(np.diff(w) > 0) and w[-1] <= 6144
    with pytest.raises(ValueError):
        sp.generate_pulse_widths(0)


def _events(rows):
    return np.array(rows, dtype=pc.EVENT_DTYPE)


def test_cluster_events(sp):
    dms = [0.0, 10.0, 20.0, 30.0, 40.0, 50.0]
    widths = [1, 2, 4, 8]
    tsamp = 1e-3
    ev = _events([
        # one pulse seen at DMs 1, 2, 3 around sample 1000: the top is DM 2
        (1, 1002, 2, 9.0), (2, 1000, 1, 15.0), (3, 998, 2, 11.0),
        # the same time, DM index 5: more than dm_gap = 1 from index 3 -> its own pulse
        (5, 1001, 3, 8.5),
        # a later group: equal S/N at DMs 0 and 1 -> the lower DM; and twice at DM 0 -> the earlier sample
        (0, 5003, 0, 12.0), (0, 5001, 1, 12.0), (1, 5000, 0, 12.0),
        # alone
        (4, 9000, 3, 20.0),
    ])
    pulses = sp.cluster_events(ev, dms, tsamp, widths=widths)
    assert [(p.idm, p.sample, p.snr, p.npoints) for p in pulses] == [
        (4, 9000, 20.0, 1), (2, 1000, 15.0, 3), (0, 5001, 12.0, 3), (5, 1001, 8.5, 1)]
    top = pulses[1]
    assert (top.dm, top.width, top.dm_lo, top.dm_hi, top.time) == (20.0, 2, 10.0, 30.0, 1000 * tsamp)
    assert pulses[2].width == 2 and pulses[2].dm_lo == 0.0 and pulses[2].dm_hi == 10.0
    # the default time radius is the largest width (8 samples): 5003 - 5000 joins, 1002 - 9000 does not;
    # a radius of 1.5 samples cuts the first group between 998 | 1000, 1001, 1002
    near = sp.cluster_events(ev, dms, tsamp, time_radius=1.5 * tsamp, widths=widths)
    assert sorted((p.idm, p.sample, p.npoints) for p in near if p.sample < 2000) == [
        (2, 1000, 2), (3, 998, 1), (5, 1001, 1)]
    # a wider DM gap joins index 5 to the pulse
    wide = sp.cluster_events(ev, dms, tsamp, dm_gap=2, widths=widths)
    assert [(p.idm, p.npoints, p.dm_hi) for p in wide if p.sample < 2000] == [(2, 4, 50.0)]
    assert sp.cluster_events(ev[:0], dms, tsamp, widths=widths) == []


def test_single_pulse_round_trip(sp):
    import riptide_amd
    assert riptide_amd.SinglePulse is sp.SinglePulse and riptide_amd.single_pulse is sp
    assert callable(riptide_amd.search_filterbank_pulses)
    p = sp.SinglePulse(time=1.25, sample=1250, dm=20.0, idm=2, width=9, snr=13.5, npoints=4, dm_lo=10.0, dm_hi=30.0)
    d = p.to_dict()
    assert set(d) == {"time", "sample", "dm", "idm", "width", "snr", "npoints", "dm_lo", "dm_hi"}
    q = sp.SinglePulse.from_dict(d)
    assert q == p and q.to_dict() == d and q is not p


def test_asan_pulse_check():
    """`make asan` builds build/asan/pulse_check (g++, AddressSanitizer +
    UBSan, no HIP): rt_single_pulse_host on exact-size heap arrays (N equal to
    the largest width, R above N, one row, ldx > N, a capacity of zero) and
    every error return."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "pulse_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("pulse_check OK")
