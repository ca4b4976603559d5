"""GPU tests of the single-pulse kernels at every path the launch plan and the
tile count select: each chunks-per-tile class of pulse_plan (named through
engine.pulse_plan, pinned by test_pulse_host.py::test_plan_table) with a tile
that has its whole halo, the offsets kernel above 1024 tiles, the tie and edge
rules across tile boundaries, non-finite samples in a neighbour's halo.  Every
comparison is bit for bit: with the host specification
(single_pulse.single_pulse_host) and, on dyadic rows, with the numpy
restatement of pulse_common as well.

Durations on an MI355X (pytest --durations=20, recorded, not asserted; the
host specification and the restatement run inside each test):

    1.63 s  setup of the first test (torch, the device)
    1.29 s  test_most_series
    0.28 s  test_many_tiles_several_per_row
    0.12 s  test_every_chunk_plan[64-64-1-2T+37] (the first launch)
    0.08 s  test_every_chunk_plan[64-64-1-5T+37], test_many_tiles[3073]
    0.05 s  test_many_tiles[2047], [2049]
    0.03 s  test_many_tiles[1024], [1025], test_ties_and_edges_on_the_device
    0.02 s  test_every_chunk_plan at (6144, 6144) and (4096, 6144, 5T+37), test_multi_chunk_stride_and_stream
    0.01 s  every other case of test_every_chunk_plan; test_special_values below 0.005 s
    29 passed in 4.3 s
"""
import numpy as np
import pytest

import pulse_common as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def ladder(wmax):
    from riptide_amd.single_pulse import generate_pulse_widths
    return np.unique(np.append(generate_pulse_widths(wmax), wmax)).astype(np.int32)


def tile_chunks(N, R, chunk):
    """The number of chunks each tile of a row works through: its outputs and
    a halo of R on each side, clipped to the row, `chunk` at a time."""
    from riptide_amd import engine
    T = engine.PULSE_TILE
    return [-(-(min(N, min(N, t0 + T) + R) - max(0, t0 - R)) // chunk) for t0 in range(0, N, T)]


def events_per_tile(ev, N):
    from riptide_amd import engine
    return np.bincount(ev["sample"] // engine.PULSE_TILE, minlength=-(-N // engine.PULSE_TILE))


# ---- 1. every chunk plan

# (wmax, R) -> chunks per full tile; the last four: the plan nearest the LDS
# limit, a chunk longer than T + 2R with a radius off the segment grid, a
# width and radius of exactly one segment, and no halo at all.  With a whole
# halo (5000, 2048), (1025, 3000), (1024, 1024) and (5000, 0) fill every one
# of the plan's chunk_segs segments; at (5000, 0) the tile's own last outputs
# read the last of them, with a halo only outputs of the halo do.
PLANS = [(64, 64, 1), (6144, 2048, 2), (6144, 4096, 3), (4096, 6144, 4), (6144, 6144, 6), (5000, 2048, 1),
         (1025, 3000, 1), (1024, 1024, 1), (5000, 0, 1)]
PLAN_THRESHOLD = 4.0


def plan_rows(make, seed, N, wmax, R, chunk):
    """Two rows with pulse_common.tile_pulses, one boxcar of about wmax / 2
    samples (S/N 2 to 4.5) centred on the first chunk boundary of tile 1 and
    of the first tile with a whole halo, and in every tile one sample of 16,
    above every S/N the rest gives (rows in turn, so that two of a row are
    more than any radius apart): an event there whatever the radius.  Still
    a multiple of 1 / 256: the sums of the dyadic rows stay exact."""
    from riptide_amd import engine
    T = engine.PULSE_TILE
    wb = max(1, wmax // 2)
    amp = 2.0 ** np.floor(np.log2(4.5 / np.sqrt(wb)))
    pulses = pc.tile_pulses(N, T)
    full = -(-R // T)                                     # the first tile with t0 - R >= 0
    for tile in sorted({1, full}):
        boundary = max(0, tile * T - R) + chunk
        pulses.append((tile, boundary - wb // 2, wb, amp))
    x = make(seed, 2, N, pulses)
    for tile, t0 in enumerate(range(0, N, T)):
        x[tile % 2, t0 + 1000 if t0 + 1000 < N - 10 else N - 10] = 16.0
    return x


def check_plan_case(torch, wmax, R, nchunks, N, **kw):
    from riptide_amd import engine
    T = engine.PULSE_TILE
    chunk, segs, lds = engine.pulse_plan(wmax, R)
    assert -(-(T + 2 * R) // chunk) == nchunks, (chunk, segs, lds)
    widths = ladder(wmax)
    assert widths[-1] == wmax
    per_tile = tile_chunks(N, R, chunk)
    for make, numpy_too in ((pc.dyadic_rows, True), (pc.gaussian_rows, False)):
        x = plan_rows(make, 100 * wmax + R, N, wmax, R, chunk)
        hev = pc.assert_device_is_host(torch, x, widths, PLAN_THRESHOLD, R, numpy_too=numpy_too, **kw)
        assert np.all(events_per_tile(hev, N) >= 1), events_per_tile(hev, N)
    return per_tile


@pytest.mark.parametrize("nkind", ["2T+37", "5T+37"])
@pytest.mark.parametrize("wmax,R,nchunks", PLANS)
def test_every_chunk_plan(torch, wmax, R, nchunks, nkind):
    """One (wmax, R) per chunks-per-tile class and the edges, at N = 2T + 37,
    where the row's ends clip every tile's halo, and at N = 5T + 37, where
    tile 2 has its whole halo at any radius and so runs the class's full
    count of chunks (at 2T + 37 the (6144, 6144) plan runs 3 of its 6)."""
    from riptide_amd import engine
    T = engine.PULSE_TILE
    N = {"2T+37": 2 * T + 37, "5T+37": 5 * T + 37}[nkind]
    per_tile = check_plan_case(torch, wmax, R, nchunks, N)
    if nkind == "5T+37":
        assert per_tile[2] == nchunks == max(per_tile), per_tile


def test_multi_chunk_stride_and_stream(torch):
    """The three-chunk plan on rows of a wider tensor (ldx = N + 3, NaN
    between the rows) and a side stream."""
    from riptide_amd import engine
    N = 2 * engine.PULSE_TILE + 37
    check_plan_case(torch, 6144, 4096, 3, N, stride_pad=3, stream=torch.cuda.Stream())


# ---- 2. many tiles

def many_rows(seed, B, N):
    """Dyadic noise; the last row has a sample of 6, so that the last tile,
    the one a short count of tiles per thread would leave out, has an event.
    No -0.0: as a row's first sample it gives best = +0.0 by the specification
    (0.0 + -0.0) and -0.0 by the restatement's whole-row cumsum, equal values
    of different bits (test_special_values has -0.0 against the host)."""
    x = pc.dyadic_rows(seed, B, N) + np.float32(0.0)
    x[-1, N // 2] = 6.0
    return x


def quiet_third(x, widths, thr, R):
    """The host events of x, having checked on the restatement that roughly a
    third of the rows (a fifth to 45 %) have no event, every other row has one
    to five and the last row has one."""
    from riptide_amd import single_pulse
    ref = pc.numpy_single_pulse(x, widths, thr, R)
    per_row = np.bincount(ref[0]["series"], minlength=x.shape[0])
    quiet = np.mean(per_row == 0)
    assert 0.2 <= quiet <= 0.45 and per_row.max() <= 5 and per_row[-1] >= 1, (quiet, per_row.max(), per_row[-1])
    host = single_pulse.single_pulse_host(x, widths, thr, radius=R, dense=True)
    pc.assert_same_results(host, ref, "host specification against the numpy restatement")
    return host


def check_many_tiles(torch, x, widths, thr, R, ntiles):
    from riptide_amd import engine
    B, N = x.shape
    assert B * -(-N // engine.PULSE_TILE) == ntiles
    host = quiet_third(x, widths, thr, R)
    key = host[0]["series"].astype(np.int64) * N + host[0]["sample"]
    assert np.all(np.diff(key) > 0)
    first = pc.run_device(torch, x, widths, thr, R)
    pc.assert_same_results(first, host, "device against the host specification")
    key = first[0]["series"].astype(np.int64) * N + first[0]["sample"]
    assert np.all(np.diff(key) > 0)
    pc.assert_same_results(pc.run_device(torch, x, widths, thr, R), first, "second run against the first")


@pytest.mark.parametrize("ntiles", [1024, 1025, 2047, 2049, 3073])
def test_many_tiles(torch, ntiles):
    """A tile per row of 70 samples around and above the 1024 threads of the
    offsets kernel: every thread sums the counts of one, two or three tiles, the
    threads past the end of none."""
    check_many_tiles(torch, many_rows(ntiles, ntiles, 70), [1, 2, 4], 2.375, 2, ntiles)


def test_many_tiles_several_per_row(torch):
    """300 rows of five tiles each: most tiles have no event."""
    from riptide_amd import engine
    check_many_tiles(torch, many_rows(300, 300, 4 * engine.PULSE_TILE + 5), [1, 2, 4], 4.0, 2, 1500)


def test_most_series(torch):
    """65535 rows, the most a call takes (a grid row each); 65536 are refused
    before any launch."""
    from riptide_amd import engine
    check_many_tiles(torch, many_rows(65535, 65535, 8), [1, 2], 1.1875, 2, 65535)
    with pytest.raises(ValueError, match="65535 series"):
        engine.single_pulse_device(torch.zeros((65536, 8), dtype=torch.float32, device="cuda"), [1, 2], 1.5, radius=2)


# ---- 3. ties and edges

def test_ties_and_edges_on_the_device(torch):
    """The plateau, pair, width-tie and edge rules where the device reads them
    across a tile boundary or from the -inf of a row's ends."""
    from riptide_amd import engine, single_pulse
    T = engine.PULSE_TILE
    N = 2 * T + 37
    R = 5
    x = np.zeros((7, N), dtype=np.float32)
    x[0, T - 2:T + 2] = 3.0                  # a plateau astride the tile boundary
    x[1, [1000, 1000 + R]] = 3.0             # equal values R apart
    x[2, [1000, 1000 + R + 1]] = 3.0         # and R + 1 apart
    x[3, [T - 1, T - 1 + R]] = 3.0           # the same, the partner in the next tile
    x[4, [T - 1, T + R]] = 3.0
    x[5, [T - 1 - R, T - 1]] = 3.0           # the partner in the tile before
    x[6, [T - 2 - R, T - 1]] = 3.0
    expected = {0: [T - 2], 1: [1000], 2: [1000, 1000 + R + 1], 3: [T - 1], 4: [T - 1, T + R], 5: [T - 1 - R],
                6: [T - 2 - R, T - 1]}
    hev = pc.assert_device_is_host(torch, x, [1], 2.0, R, numpy_too=True)
    for row, samples in expected.items():
        assert hev[hev["series"] == row]["sample"].tolist() == samples, row
    assert np.all(hev["snr"] == 3.0) and np.all(hev["iwidth"] == 0)

    # widths 1 and 4 tie at sample T + 2 (2 / sqrt(1) = 4 / sqrt(4)): the smaller width
    y = np.zeros((1, N), dtype=np.float32)
    y[0, T:T + 4] = [0.5, 0.5, 2.0, 1.0]
    hev = pc.assert_device_is_host(torch, y, [1, 4], 1.5, 12, numpy_too=True)
    assert hev["sample"].tolist() == [T + 2] and hev["iwidth"].tolist() == [0] and hev["snr"].tolist() == [2.0]

    # a smallest width of 4: no width fits at the first two samples and the last, -inf in every tile's halo
    z = pc.dyadic_rows(41, 2, N, pc.tile_pulses(N, T))
    z[1] = 0.0
    z[1, 1:5] = 2.0                          # best[3] = 4, with the -inf of samples 0 and 1 in its neighbourhood
    z[1, N - 5:N - 1] = 2.0                  # best[N - 3] = 4, with that of sample N - 1
    z[1, T - 2:T + 2] = 2.0                  # best[T] = 4
    for radius in (R, 64):
        got = pc.run_device(torch, z, [4, 10], 1.0, radius)
        pc.assert_same_results(got, single_pulse.single_pulse_host(z, [4, 10], 1.0, radius=radius, dense=True),
                               "device against the host specification")
        pc.assert_same_results(got, pc.numpy_single_pulse(z, [4, 10], 1.0, radius),
                               "device against the numpy restatement")
        ev, best, kbest = got
        for row in range(2):
            assert np.flatnonzero(kbest[row] == -1).tolist() == [0, 1, N - 1]
            assert np.flatnonzero(best[row] == -np.inf).tolist() == [0, 1, N - 1]
        assert ev[ev["series"] == 1]["sample"].tolist() == [3, T, N - 3]

    # one sample
    one = np.full((3, 1), 3.0, dtype=np.float32)
    one[1, 0] = 1.0
    for radius in (0, R):
        hev = pc.assert_device_is_host(torch, one, [1], 2.0, radius, numpy_too=True)
        assert hev["series"].tolist() == [0, 2] and hev["sample"].tolist() == [0, 0]

    # radius 0: no halo, every sample at or above the threshold is an event
    widths = single_pulse.generate_pulse_widths(64)
    for make, numpy_too in ((pc.gaussian_rows, False), (pc.dyadic_rows, True)):
        g = make(43, 1, N, pc.tile_pulses(N, T))
        hev = pc.assert_device_is_host(torch, g, widths, 1.0, 0, numpy_too=numpy_too)
        hbest = single_pulse.single_pulse_host(g, widths, 1.0, radius=0, dense=True)[1]
        assert hev["sample"].tolist() == np.flatnonzero(hbest[0] >= 1.0).tolist() and hev.size > 4096


# ---- 4. special values

@pytest.mark.parametrize("R", [1, 64])
def test_special_values(torch, R):
    """A NaN three samples before the tile boundary (tile 0's own, and in the
    halo segment of tile 1), +Inf, -Inf, -0.0 and a denormal at a segment's
    first sample: the host specification's bits (the numpy restatement sums
    the whole row and differs after a NaN)."""
    from riptide_amd import engine, single_pulse
    T = engine.PULSE_TILE
    N = 2 * T + 37
    widths = single_pulse.generate_pulse_widths(64)
    wmax = int(widths[-1])
    x = pc.gaussian_rows(47, 1, N, pc.tile_pulses(N, T))
    x[0, T - 3] = np.nan
    x[0, 100] = np.inf
    x[0, 3000] = -np.inf
    x[0, 1024] = -0.0
    x[0, 2048] = 1e-40
    x[0, 6000] = -0.0
    x[0, 6001] = 1e-40
    assert 0.0 < x[0, 2048] < np.finfo(np.float32).tiny
    got = pc.run_device(torch, x, widths, 3.0, R)
    pc.assert_same_results(got, single_pulse.single_pulse_host(x, widths, 3.0, radius=R, dense=True),
                           "device against the host specification")
    ev, best, kbest = got
    assert not np.any(np.isnan(best))
    assert best[0, T - 3] == -np.inf and kbest[0, T - 3] == -1
    # the partial sums restart at the segment after the NaN
    clean = 1024 * -(-(T - 2) // 1024) + wmax // 2
    assert np.all(np.isfinite(best[0, clean:]))
    assert np.any(ev["sample"] >= clean) and not np.any(np.isnan(ev["snr"]))
