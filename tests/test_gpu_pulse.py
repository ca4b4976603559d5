"""GPU tests of the single-pulse search: engine.single_pulse_device against the
host specification (single_pulse.single_pulse_host), bit for bit, at the
shapes where the tile kernel changes path; the event buffer's capacity rules;
the filterbank front end; and `pulses=` of EngineSearcher.search_filterbank."""
import numpy as np
import pytest

import dedisp_common as dc
import pulse_common as pc

pytestmark = pytest.mark.gpu

DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def to_host(ev):
    from riptide_amd.single_pulse import events_to_host
    return events_to_host(ev)


assert_device_is_host = pc.assert_device_is_host
tile_pulses = pc.tile_pulses


def with_end_events(x):
    """Rows 0 and 1 (or row 0 alone) quiet at their ends but for one sample
    of 4 at the very first and the very last place: with a radius of 1 those
    are events."""
    x[:2, :8] = 0.0
    x[:2, -8:] = 0.0
    x[0, 0] = 4.0
    x[-1 if x.shape[0] == 1 else 1, -1] = 4.0
    return x


@pytest.mark.parametrize("R", ["one", "wmax", "limit"])
@pytest.mark.parametrize("nkind", ["wmax", "T-1", "T", "T+1", "2T+37"])
def test_device_equals_host(torch, nkind, R):
    """N around the tile length T and at the largest width, one row and five,
    dyadic and Gaussian samples, radius 1, the largest width and the limit."""
    from riptide_amd import engine, single_pulse
    T, L = engine.PULSE_TILE, engine.PULSE_MAX_WIDTH
    widths = single_pulse.generate_pulse_widths(64)
    wmax = int(widths[-1])
    N = {"wmax": wmax, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+37": 2 * T + 37}[nkind]
    radius = {"one": 1, "wmax": wmax, "limit": L}[R]
    for B, make, seed in ((1, pc.dyadic_rows, 1), (5, pc.dyadic_rows, 2), (5, pc.gaussian_rows, 3)):
        x = with_end_events(make(seed * 1000 + N, B, N, tile_pulses(N, T)))
        hev = assert_device_is_host(torch, x, widths, 3.0, radius)
        assert hev.size > 0
        if radius == 1:
            # an event at the first and at the last valid sample
            assert hev[hev["series"] == 0]["sample"][0] == 0
            assert hev[hev["series"] == min(1, B - 1)]["sample"][-1] == N - 1


@pytest.mark.parametrize("N", ["wmax", "2T+37"])
def test_widest_ladder(torch, N):
    """Every width of the ladder up to RT_PULSE_MAX_WIDTH (the most widths a
    default ladder has) with the radius at the limit: windows that hold whole
    segments of the partial sums, the tile worked through in chunks."""
    from riptide_amd import engine, single_pulse
    T, L = engine.PULSE_TILE, engine.PULSE_MAX_WIDTH
    widths = np.append(single_pulse.generate_pulse_widths(L), L).astype(np.int32)
    widths = np.unique(widths)
    n = L if N == "wmax" else 2 * T + 37
    pulses = tile_pulses(n, T) + [(0, 500, 3000, 0.25), (1, T - 600, 1100, 0.25)]
    for make in (pc.dyadic_rows, pc.gaussian_rows):
        x = make(n, 2, n, pulses)
        assert_device_is_host(torch, x, widths, 4.0, L)
        assert_device_is_host(torch, x, widths, 4.0, 1)


def test_one_width_stride_and_stream(torch):
    """One width only (1, and an odd one); rows of a wider tensor read in
    place (ldx > N, NaN between the rows); a non-default stream."""
    from riptide_amd import engine, single_pulse
    T = engine.PULSE_TILE
    N = 2 * T + 37
    x = pc.gaussian_rows(77, 5, N, tile_pulses(N, T))
    for w in ([1], [7]):
        assert_device_is_host(torch, x, w, 3.5, 16)
    widths = single_pulse.generate_pulse_widths(64)
    assert_device_is_host(torch, x, widths, 3.5, 64, stride_pad=5)
    assert_device_is_host(torch, x, widths, 3.5, 64, stream=torch.cuda.Stream(), stride_pad=3)
    # a 1-D series
    ev = engine.single_pulse_device(torch.from_numpy(x[2]).cuda(), widths, 3.5)
    assert pc.events_equal(to_host(ev), single_pulse.single_pulse_host(x[2], widths, 3.5))


def test_capacity(torch):
    """A first buffer too small for the events still gives the complete,
    sorted list; more than max_events raises; two runs are identical."""
    from riptide_amd import engine, single_pulse
    T = engine.PULSE_TILE
    N = 2 * T + 37
    widths = single_pulse.generate_pulse_widths(64)
    x = pc.gaussian_rows(5, 5, N, tile_pulses(N, T))
    hev = assert_device_is_host(torch, x, widths, 0.5, 1, capacity=16)
    assert hev.size > 5000
    assert_device_is_host(torch, x, widths, 0.5, 1, capacity=0)
    d = torch.from_numpy(x).cuda()
    with pytest.raises(ValueError, match="threshold 0.5"):
        engine.single_pulse_device(d, widths, 0.5, radius=1, max_events=1000)
    a = engine.single_pulse_device(d, widths, 0.5, radius=1, dense=True)
    b = engine.single_pulse_device(d, widths, 0.5, radius=1, dense=True)
    for u, v in zip(list(a[0]) + list(a[1:]), list(b[0]) + list(b[1:])):
        assert torch.equal(u, v)
    # argument checks, before any launch
    with pytest.raises(ValueError, match="strictly ascending"):
        engine.single_pulse_device(d, [2, 2], 8.0)
    with pytest.raises(ValueError, match="RT_PULSE_MAX_WIDTH"):
        engine.single_pulse_device(d, [1, 2], 8.0, radius=engine.PULSE_MAX_WIDTH + 1)
    with pytest.raises(ValueError, match="finite"):
        engine.single_pulse_device(d, [1, 2], float("inf"))
    with pytest.raises(ValueError, match="float32"):
        engine.single_pulse_device(d.double(), [1, 2], 8.0)


# ---- the filterbank front end

DMS = [0.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 70.0]
TRUE_DM = 3
TRUTH = [(3000, 1), (8000, 8), (12000, 40)]      # (sample at the top of the band, width)
NCHANS, NSAMP = 64, 16384


def inject(x, amps):
    sweep = dc.numpy_delays(dc.band(NCHANS), [DMS[TRUE_DM]], dc.TSAMP)[0]
    for (t0, w), a in zip(TRUTH, amps):
        for c in range(NCHANS):
            x[t0 + int(sweep[c]):t0 + int(sweep[c]) + w, c] += a
    return x


def header(nbits):
    return {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": dc.TSAMP,
            "nbits": nbits, "fch1": 400.0, "foff": -32.0 / NCHANS, "nchans": NCHANS, "nifs": 1}


@pytest.fixture(scope="module")
def fil8(tmp_path_factory):
    """uint8 noise of sigma 10 per channel (80 after the sum over 64
    channels); pulses of S/N 64 a sqrt(w) / 80 = 24, 27 and 25."""
    from riptide_amd.reading import write_sigproc
    rng = np.random.RandomState(2468)
    x = inject(rng.normal(100.0, 10.0, size=(NSAMP, NCHANS)), (30.0, 12.0, 5.0))
    x = np.clip(np.round(x), 0, 255).astype(np.uint8)
    path = str(tmp_path_factory.mktemp("pulse") / "eight.fil")
    write_sigproc(path, x, header(8))
    return path


def assert_recovered(pulses, widths):
    assert len(pulses) >= 3
    top = sorted(pulses[:3], key=lambda p: p.sample)
    assert all(p.snr > 12.0 for p in top), top
    if len(pulses) > 3:
        assert pulses[3].snr < min(p.snr for p in top)
    for p, (t0, w) in zip(top, TRUTH):
        assert abs(p.idm - TRUE_DM) <= 1, p
        assert abs(p.sample - (t0 + w // 2)) <= w, p
        k_true = int(np.argmin(np.abs(np.asarray(widths) - w)))
        k_got = int(np.flatnonzero(np.asarray(widths) == p.width)[0])
        assert abs(k_got - k_true) <= 1, p
        assert p.dm == DMS[p.idm] and p.time == p.sample * dc.TSAMP and p.dm_lo <= p.dm <= p.dm_hi


def test_search_filterbank_pulses(torch, fil8):
    """Three dispersed pulses of widths 1, 8 and 40 injected at one DM come
    back as the top three pulses, and the events are the host specification's
    on the device's own normalised series."""
    import riptide_amd
    from riptide_amd import engine, single_pulse
    from riptide_amd.dedispersion import dedisperse_filterbank
    pulses, events = riptide_amd.search_filterbank_pulses(fil8, DMS, DEREDDEN, batch=3)
    widths = single_pulse.generate_pulse_widths(512)
    assert_recovered(pulses, widths)
    fb = riptide_amd.open_filterbank(fil8)
    series = dedisperse_filterbank(fb, DMS)
    x = engine.deredden_normalise(series, int(round(DEREDDEN["rmed_width"] / fb.tsamp)), DEREDDEN["rmed_minpts"])
    ref = single_pulse.single_pulse_host(x.cpu().numpy(), widths, 8.0)
    assert pc.events_equal(events, ref)
    assert pulses == single_pulse.cluster_events(ref, DMS, fb.tsamp)


def test_two_bit_and_zero_dm(torch, fil8, tmp_path):
    """A PackedFilterbank (2-bit) and zero_dm=True run through the same call
    and recover the same three pulses."""
    import riptide_amd
    from riptide_amd import single_pulse
    from riptide_amd.reading import PackedFilterbank, pack_samples, write_sigproc
    widths = single_pulse.generate_pulse_widths(512)
    rng = np.random.RandomState(1357)
    x = inject(rng.normal(1.5, 0.8, size=(NSAMP, NCHANS)), (2.0, 1.0, 0.5))
    x = np.clip(np.round(x), 0, 3).astype(np.uint8)
    path = str(tmp_path / "two.fil")
    write_sigproc(path, pack_samples(x, 2).ravel(), header(2))
    fb = riptide_amd.open_filterbank(path)
    assert isinstance(fb, PackedFilterbank)
    pulses, _ = riptide_amd.search_filterbank_pulses(fb, DMS, DEREDDEN)
    assert_recovered(pulses, widths)
    pulses, _ = riptide_amd.search_filterbank_pulses(fil8, DMS, DEREDDEN, zero_dm=True)
    assert_recovered(pulses, widths)


RANGES = [{"name": "short", "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
           "find_peaks": {"smin": 6.0}}]


def test_searcher_pulses_keyword(torch, fil8):
    """pulses=None leaves EngineSearcher.search_filterbank as it was; with
    parameters the peak lists are unchanged and the pulses are
    search_filterbank_pulses'; dispatch.search_filterbank passes them on."""
    import riptide_amd
    from riptide_amd.dispatch import EngineSearcher
    fb = riptide_amd.open_filterbank(fil8)
    searcher = EngineSearcher(DEREDDEN, RANGES, device=0, batch=3)
    plain = searcher.search_filterbank(fb, DMS)
    assert isinstance(plain, list) and len(plain) == len(DMS)
    same = searcher.search_filterbank(fb, DMS, pulses=None)
    both = searcher.search_filterbank(fb, DMS, pulses={"threshold": 8.0})
    assert isinstance(both, tuple) and len(both) == 2
    as_tuples = lambda per: [[tuple(p) for p in plist] for plist in per]
    assert as_tuples(same) == as_tuples(plain) and as_tuples(both[0]) == as_tuples(plain)
    ref, ref_events = riptide_amd.search_filterbank_pulses(fb, DMS, DEREDDEN, batch=3)
    assert both[1] == ref and len(ref) >= 3
    assert pc.events_equal(searcher.pulse_events, ref_events)
    flat = riptide_amd.search_filterbank(fb, DMS, searcher)
    peaks, pulses = riptide_amd.search_filterbank(fb, DMS, searcher, pulses={"threshold": 8.0})
    assert [tuple(p) for p in peaks] == [tuple(p) for p in flat] and pulses == ref
