"""Signal injection on the device: engine.inject_device against the host
specification bit for bit at every shape, kind, factor and edge, on a side
stream and between canary rows; inject= of the dedispersion entry points
against files written from inject_host's samples; inject_filterbank; and
pulsars and a pulse found where they were injected."""
import numpy as np
import pytest

import dedisp_common as dc
import inject_common as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _device_inject(torch, x, T, t_origin, seed, stream=None, pad=3):
    """inject_device on x between `pad` canary rows: (result, canaries intact)."""
    from riptide_amd import engine
    g, n = x.shape
    fill = 7 if x.dtype != np.float32 else -12345.0
    wide = np.full((g + 2 * pad, n), fill, dtype=x.dtype)
    wide[pad:pad + g] = x
    d = torch.from_numpy(wide).cuda()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    engine.inject_device(d[pad:pad + g], T, t_origin, seed, stream=stream)
    if stream is not None:
        stream.synchronize()
    back = d.cpu().numpy()
    return back[pad:pad + g], bool(np.all(back[:pad] == fill) and np.all(back[pad + g:] == fill))


@pytest.mark.parametrize("nchans", ic.NCHANS)
@pytest.mark.parametrize("dtype", ic.DTYPES)
def test_device_equals_host(torch, dtype, nchans):
    """Bit for bit over g (one row, ragged and whole tiles of rows, several
    workgroups), t_origin, K, and log2bins on both sides of 2^12, with zero
    and non-zero factors in one call, pulse windows across both ends of the
    block, delays larger than it, and the rows around the block untouched
    (with 3 canary rows in front an 8-bit block of odd nchans starts off a
    dword boundary)."""
    from riptide_amd.injection import inject_host
    for g in (1, 63, 64, 257, 1000):
        x = ic.block(g, nchans, dtype)
        for t_origin in (0, 1000):
            for K, log2bins in ((1, 1), (3, 10), (17, 12), (3, 13), (17, 16)):
                T = ic.tables(K, nchans, g, t_origin, log2bins)
                want = inject_host(x, T, t_origin, seed=5)
                got, intact = _device_inject(torch, x, T, t_origin, 5)
                assert got.tobytes() == want.tobytes(), (g, t_origin, K, log2bins)
                assert intact, (g, t_origin, K, log2bins)


@pytest.mark.parametrize("dtype", ["uint8", "int8"])
def test_saturation(torch, dtype):
    from riptide_amd.injection import inject_host
    x, cases = ic.saturation_case(dtype)
    for T in cases:
        got, intact = _device_inject(torch, x, T, 0, 1)
        assert intact and got.tobytes() == inject_host(x, T, seed=1).tobytes()


def test_side_stream_seed_and_errors(torch):
    from riptide_amd import engine
    from riptide_amd.injection import inject_host
    g, n = 257, 65
    x = ic.block(g, n, "uint8")
    T = ic.tables(3, n, g, 0, 10)
    side = torch.cuda.Stream()
    got, intact = _device_inject(torch, x, T, 0, 11, stream=side)
    assert intact and got.tobytes() == inject_host(x, T, 0, seed=11).tobytes()
    other, _ = _device_inject(torch, x, T, 0, 12)
    assert other.tobytes() == inject_host(x, T, 0, seed=12).tobytes() and other.tobytes() != got.tobytes()
    # no signal: nothing launched, nothing changed
    same, _ = _device_inject(torch, x, ic.tables(0, n, g, 0, 1), 0, 1)
    assert same.tobytes() == x.tobytes()
    d = torch.from_numpy(x).cuda()
    with pytest.raises(ValueError, match="65 channels"):
        engine.inject_device(d[:, :64].contiguous(), T)
    with pytest.raises(ValueError, match="2\\^31"):
        engine.inject_device(d, T, t_origin=(1 << 31) - g)
    with pytest.raises(ValueError, match="contiguous"):
        engine.inject_device(d[:, ::2], T)
    assert d.cpu().numpy().tobytes() == x.tobytes()


# ---------------------------------------------------------------- through the file-level entry points

def _noise_file(path, dtype, nchans, nsamp, seed):
    rng = np.random.RandomState(seed)
    x = rng.normal(100.0, 10.0, size=(nsamp, nchans))
    x = x.astype(np.float32) if dtype == "float32" else np.clip(np.round(x), 0, 255).astype(np.uint8)
    return x, ic.write_filterbank(path, x)


def _file_tables(fb, span, accel=0.0):
    from riptide_amd.injection import PulsarSignal, PulseSignal, injection_tables
    sig = [PulsarSignal(0.25, 15.0, 40.0, accel=accel), PulseSignal(1.5, 10.0, 30.0, 0.01)]
    return injection_tables(sig, fb.freqs, fb.tsamp, span, 10.0)


@pytest.mark.parametrize("dtype,nchans", [("uint8", 64), ("float32", 130), ("uint8", 65)])
def test_dedisperse_filterbank_inject(torch, tmp_path, dtype, nchans):
    """inject= equals the same call on a file holding inject_host's samples,
    at two gulps, and with a block mask: the injection comes first."""
    from riptide_amd import rfi
    from riptide_amd.dedispersion import (dedisperse_filterbank, dedisperse_filterbank_plan, dispersion_delays,
                                          dm_plan)
    from riptide_amd.injection import inject_filterbank, inject_host
    from riptide_amd.reading import Filterbank
    nsamp, dms = 4000, [0.0, 10.0, 15.0, 30.0]
    x, fname = _noise_file(tmp_path / "n.fil", dtype, nchans, nsamp, 3)
    fb = Filterbank(fname)
    _, max_delay = dispersion_delays(fb.freqs, dms, fb.tsamp)
    T = _file_tables(fb, nsamp - max_delay)
    y = inject_host(x, T, seed=21)
    assert y.tobytes() != x.tobytes()
    fy = Filterbank(ic.write_filterbank(tmp_path / "y.fil", y))
    want = dedisperse_filterbank(fy, dms).cpu().numpy()
    for gulp in (None, 1009, max_delay + 1):
        got = dedisperse_filterbank(fb, dms, inject=(T, 21), gulp=gulp).cpu().numpy()
        assert got.tobytes() == want.tobytes(), gulp
    assert dedisperse_filterbank(fb, dms, inject=T).cpu().numpy().tobytes() == \
        dedisperse_filterbank(Filterbank(ic.write_filterbank(tmp_path / "y0.fil", inject_host(x, T))), dms) \
        .cpu().numpy().tobytes()
    # the block mask flags cells of the injected file and is applied behind the injection
    cells = np.zeros((nsamp // 256 + 1, nchans), dtype=bool)
    cells[3:6, 5 % nchans] = cells[9, :: 7] = True
    fill = np.full(nchans, 100.0)
    bm = rfi.BlockMask(cells, 256, fill)
    masked = dedisperse_filterbank(fy, dms, block_mask=bm).cpu().numpy()
    both = dedisperse_filterbank(fb, dms, block_mask=bm, inject=(T, 21), gulp=1009).cpu().numpy()
    assert both.tobytes() == masked.tobytes() and masked.tobytes() != want.tobytes()
    # the plan form
    plan = dm_plan(fb.freqs, fb.tsamp, 30.0, wmin=4e-3, max_downsamp=4)
    ref = dedisperse_filterbank_plan(fy, plan)
    for gulp in (None, 1200):
        got = dedisperse_filterbank_plan(fb, plan, inject=(T, 21), gulp=gulp)
        assert len(got) == len(ref) > 0
        for a, b in zip(got, ref):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), gulp
    # and the written file
    used = inject_filterbank(fb, T, str(tmp_path / "w.fil"), seed=21, gulp=777)
    assert used is T
    fw = Filterbank(str(tmp_path / "w.fil"))
    assert np.asarray(fw.data).tobytes() == y.tobytes() and dict(fw.header) == dict(fb.header)


# ---------------------------------------------------------------- end to end
E2E_NCHANS, E2E_NSAMP = 64, 1 << 15
E2E_DMS = [0.0, 10.0, 20.0, 30.0, 40.0]
E2E_DM, E2E_PERIOD = 20.0, 0.5
E2E_DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}
E2E_RANGES = [{"name": "short",
               "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
               "find_peaks": {"smin": 7.0}}]


@pytest.fixture(scope="module")
def e2e(torch, tmp_path_factory):
    """(Filterbank of seeded Gaussian uint8 noise, 64 x 2^15, the span the DM list leaves)."""
    from riptide_amd.dedispersion import dispersion_delays
    from riptide_amd.reading import Filterbank
    _, fname = _noise_file(tmp_path_factory.mktemp("inj") / "e2e.fil", "uint8", E2E_NCHANS, E2E_NSAMP, 77)
    fb = Filterbank(fname)
    _, max_delay = dispersion_delays(fb.freqs, E2E_DMS, fb.tsamp)
    return fb, E2E_NSAMP - max_delay


def test_injected_pulsar_is_found(e2e):
    """snr = 30 at DM 20, period 0.5 s: the top peak of search_filterbank is at
    the injected DM trial, its period within two steps of the trial grid (the
    rule of test_gpu_dedisp.py: a step is at most the drift of one phase bin
    over the observation, p * (p / bins_min) / tobs).  Without inject= the
    noise has no peak there."""
    import riptide_amd
    from riptide_amd.dispatch import EngineSearcher
    from riptide_amd.injection import PulsarSignal, injection_tables
    fb, span = e2e
    T = injection_tables(PulsarSignal(E2E_PERIOD, E2E_DM, 30.0, ducy=0.03), fb.freqs, fb.tsamp, span, 10.0)
    searcher = EngineSearcher(E2E_DEREDDEN, E2E_RANGES, device=0, batch=4)
    peaks = riptide_amd.search_filterbank(fb, E2E_DMS, searcher, inject=(T, 1))
    best = max(peaks, key=lambda p: p.snr)
    print("best:", best)
    assert best.dm == E2E_DM
    step = E2E_PERIOD * (E2E_PERIOD / 240) / (E2E_NSAMP * dc.TSAMP)
    assert abs(best.period - E2E_PERIOD) <= 2 * step, best
    plain = riptide_amd.search_filterbank(fb, E2E_DMS, searcher)
    assert not [p for p in plain if abs(p.period - E2E_PERIOD) <= 2 * step and p.snr > 0.5 * best.snr]


def test_injected_accelerated_pulsar_is_found(e2e):
    """The same with an acceleration whose drift at mid-observation is four
    pulse widths: the brightest member of the top cluster of
    search_filterbank_accel has accel within one step of the injected value."""
    import riptide_amd
    from riptide_amd import acceleration as ac
    from riptide_amd.dispatch import EngineSearcher
    from riptide_amd.injection import PulsarSignal, injection_tables
    fb, span = e2e
    tobs = span * fb.tsamp
    ducy = 0.03
    a = 4 * ducy * E2E_PERIOD * 8.0 * 299792458.0 / tobs ** 2
    trials = [-2 * a, -a, 0.0, a, 2 * a]
    T = injection_tables(PulsarSignal(E2E_PERIOD, E2E_DM, 30.0, ducy=ducy, accel=a), fb.freqs, fb.tsamp, span, 10.0)
    searcher = EngineSearcher(E2E_DEREDDEN, E2E_RANGES, device=0, batch=4)
    peaks = riptide_amd.search_filterbank_accel(fb, E2E_DMS, trials, searcher, inject=(T, 2))
    _, clusters = ac.cluster_peaks(peaks, 0.2, tobs)
    top = max(clusters, key=lambda c: max(p.snr for p in c))
    best = max(top, key=lambda p: p.snr)
    print("best:", best)
    assert best.dm == E2E_DM and abs(best.accel - a) <= a
    assert abs(best.freq - 1.0 / E2E_PERIOD) <= 0.2 / tobs


def test_injected_pulse_is_found(e2e):
    """A PulseSignal through search_filterbank_pulses: one SinglePulse at the
    injected DM trial, its time within the pulse's width of the arrival at the
    top of the band (time is given at infinite frequency)."""
    from riptide_amd.dedispersion import KDM
    from riptide_amd.injection import PulseSignal, injection_tables
    from riptide_amd.single_pulse import search_filterbank_pulses
    fb, span = e2e
    sig = PulseSignal(12.0, E2E_DM, 30.0, 0.016)
    T = injection_tables(sig, fb.freqs, fb.tsamp, span, 10.0)
    pulses, events = search_filterbank_pulses(fb, E2E_DMS, E2E_DEREDDEN, threshold=8.0, inject=(T, 3))
    print("pulses:", pulses)
    arrival = sig.time + KDM * sig.dm * fb.freqs.max() ** -2.0
    mine = [p for p in pulses if abs(p.time - arrival) <= sig.width]
    assert len(mine) == 1 and mine[0].dm == E2E_DM
    assert max(pulses, key=lambda p: p.snr) is mine[0]
    none, _ = search_filterbank_pulses(fb, E2E_DMS, E2E_DEREDDEN, threshold=8.0)
    assert not [p for p in none if abs(p.time - arrival) <= sig.width]
