"""GPU tests of the RFI kernels (csrc/dedisp_kernels.hip: row mean, zero-DM
transposes, channel statistics) and of what is built on them: the zero_dm
argument of the dedispersion and search calls, and riptide_amd.rfi.  The
device is compared with the numpy restatement of rfi_common: the mean series
bit for bit for 8-bit data, the sums within rfi_common.zero_dm_bound."""
import math

import numpy as np
import pytest

import dedisp_common as dc
import rfi_common as rc

pytestmark = pytest.mark.gpu

DMS = {1: [37.0],
       5: [0.0, 50.0, 12.5, 50.0, 3.0],
       33: list(np.random.RandomState(33).permutation(np.linspace(0.0, 50.0, 31))) + [50.0, 0.0]}
DTYPES = [np.uint8, np.int8, np.float32]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _mask_tensor(torch, mask):
    return None if mask is None else torch.from_numpy(np.asarray(mask, dtype=np.uint8)).cuda()


def run_block(torch, x, delays, max_delay, mask=None, **kw):
    """engine.dedisperse_device on the whole of x as one block -> numpy."""
    from riptide_amd import engine
    block = torch.from_numpy(x).cuda()
    d = torch.from_numpy(delays.astype(np.int32)).cuda()
    return engine.dedisperse_device(block, d, max_delay, mask=_mask_tensor(torch, mask), **kw).cpu().numpy()


def run_mean(torch, x, mask=None):
    from riptide_amd import engine
    return engine.zero_dm_mean_device(torch.from_numpy(x).cuda(), mask=_mask_tensor(torch, mask)).cpu().numpy()


def assert_mean(m, x, mask=None):
    """Bit for bit for 8-bit data.  float32: within 2^-23 |m| of the float64
    restatement -- another summation order moves the float64 quotient by far
    less than a float32 ulp, so across one rounding boundary at most."""
    ref = rc.numpy_zero_dm_mean(x, mask)
    assert m.dtype == np.float32 and m.shape == ref.shape
    if x.dtype == np.float32:
        assert np.all(np.abs(m.astype(np.float64) - ref) <= 2.0 ** -23 * np.abs(ref))
    else:
        assert np.array_equal(m, ref)


def _masks(nchans):
    """None; first, last and middle; all but one."""
    if nchans < 3:
        return [None]
    some = np.zeros(nchans, dtype=bool)
    some[[0, nchans // 2, nchans - 1]] = True
    one = np.ones(nchans, dtype=bool)
    one[nchans // 3] = False
    return [None, some, one]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nchans", [1, 3, 37, 64, 65, 257])
def test_row_mean(torch, nchans, dtype):
    """Channel counts below, at and above a wave and the 64-channel tile;
    1, 255 and 1000 time samples (a lone row, a workgroup's 16 rows not
    dividing the block); with and without a mask; all but one channel masked:
    the mean of an 8-bit block is then that channel."""
    for nsamp in (1, 255, 1000):
        x = dc.samples(np.random.RandomState(nchans + nsamp), nsamp, nchans, dtype)
        for mask in _masks(nchans):
            m = run_mean(torch, x, mask)
            assert_mean(m, x, mask)
            if mask is not None and (~mask).sum() == 1 and dtype != np.float32:
                assert np.array_equal(m, x[:, nchans // 3].astype(np.float32))
    every = np.ones(nchans, dtype=bool)
    assert not run_mean(torch, x, every).any()


@pytest.mark.parametrize("ndm", [1, 5, 33])
@pytest.mark.parametrize("nchans", [1, 3, 37, 64, 65, 257])
def test_zero_dm_channel_and_dm_tiles(torch, nchans, ndm):
    """The shapes of test_gpu_dedisp.test_channel_and_dm_tiles with the flag,
    every sample type."""
    from riptide_amd.dedispersion import dispersion_delays
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS[ndm], dc.TSAMP)
    rng = np.random.RandomState(nchans * 100 + ndm)
    nout = 300
    for dtype in DTYPES:
        x = dc.samples(rng, max_delay + nout, nchans, dtype)
        out = run_block(torch, x, delays, max_delay, zero_dm=True)
        rc.assert_zero_dm_dedispersed(out, x, delays, nout)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nout", [1, 255, 256, 257, 1000])
def test_zero_dm_time_tiles(torch, nout, dtype):
    """The shapes of test_gpu_dedisp.test_time_tiles with the flag."""
    from riptide_amd.dedispersion import dispersion_delays
    nchans = 37
    delays, max_delay = dispersion_delays(dc.band(nchans, ascending=True), DMS[5], dc.TSAMP)
    x = dc.samples(np.random.RandomState(nout), max_delay + nout, nchans, dtype)
    out = run_block(torch, x, delays, max_delay, zero_dm=True)
    assert out.shape == (5, nout)
    rc.assert_zero_dm_dedispersed(out, x, delays, nout)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dm0_is_zero(torch, dtype):
    """DM 0 sums x - m over the very channels m is the mean of: every output
    is within the bound of 0; one unmasked 8-bit channel is its own mean, so
    the output is exactly 0 at every DM."""
    from riptide_amd.dedispersion import dispersion_delays
    nchans, nout = 37, 300
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS[5], dc.TSAMP)
    x = dc.samples(np.random.RandomState(21), max_delay + nout, nchans, dtype)
    out = run_block(torch, x, delays, max_delay, zero_dm=True)
    _, mag, magm = rc.numpy_zero_dm_dedisperse(x, rc.numpy_zero_dm_mean(x), delays, nout)
    bound = rc.zero_dm_bound(x, delays, mag, magm)
    assert np.all(np.abs(out[0]) <= bound[0])
    if dtype != np.float32:
        one = np.ones(nchans, dtype=bool)
        one[20] = False
        assert not run_block(torch, x, delays, max_delay, mask=one, zero_dm=True).any()
    every = np.ones(nchans, dtype=bool)
    assert not run_block(torch, x, delays, max_delay, mask=every, zero_dm=True).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_dm_masks(torch, dtype):
    """First, last, both, all but one channel masked: the masked channels
    enter neither m nor the sum (poisoned with the largest value, they would
    move m)."""
    from riptide_amd.dedispersion import dispersion_delays
    nchans, nout = 37, 300
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS[5], dc.TSAMP)
    x = dc.samples(np.random.RandomState(4), max_delay + nout, nchans, dtype)
    first, last, both, one = (np.zeros(nchans, dtype=bool) for _ in range(4))
    first[0] = last[-1] = True
    both[[0, -1]] = True
    one[:] = True
    one[20] = False
    for mask in (first, last, both, one):
        out = run_block(torch, x, delays, max_delay, mask=mask, zero_dm=True)
        rc.assert_zero_dm_dedispersed(out, x, delays, nout, mask)
        poisoned = x.copy()
        poisoned[:, mask] = 1e30 if dtype == np.float32 else np.iinfo(dtype).max
        assert_mean(run_mean(torch, poisoned, mask), x, mask)
        assert np.array_equal(run_block(torch, poisoned, delays, max_delay, mask=mask, zero_dm=True), out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_dm_delay_spread_wider_than_the_tile(torch, dtype):
    """DMs 0 and 250 in one DM tile (test_gpu_dedisp's wide-spread case): with
    the flag 8-bit data meets the 264-sample float span too, so the direct
    path runs for 8-bit input."""
    from riptide_amd.dedispersion import dispersion_delays
    nchans = 40
    delays, max_delay = dispersion_delays(dc.band(nchans), [0.0, 250.0, 3.0, 100.0], dc.TSAMP)
    assert max_delay > 1100
    nout = 700
    x = dc.samples(np.random.RandomState(9), max_delay + nout, nchans, dtype)
    out = run_block(torch, x, delays, max_delay, zero_dm=True)
    rc.assert_zero_dm_dedispersed(out, x, delays, nout)


def test_no_over_read(torch):
    """The block is the first rows of a larger allocation whose rest is poison
    (NaN for float32; 255 behind an all-zero block for uint8): nothing of it
    reaches m, out or the statistics."""
    from riptide_amd import engine
    from riptide_amd.dedispersion import dispersion_delays
    nchans, nout = 37, 257
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS[5], dc.TSAMP)
    nsamp = max_delay + nout
    d = torch.from_numpy(delays.astype(np.int32)).cuda()
    x = dc.samples(np.random.RandomState(8), nsamp, nchans, np.float32)
    big = torch.full((nsamp + 300, nchans), float("nan"), dtype=torch.float32, device="cuda")
    big[:nsamp] = torch.from_numpy(x).cuda()
    m = engine.zero_dm_mean_device(big[:nsamp]).cpu().numpy()
    assert m.shape == (nsamp,) and np.all(np.isfinite(m))
    assert np.array_equal(m, run_mean(torch, x))
    out = engine.dedisperse_device(big[:nsamp], d, max_delay, zero_dm=True).cpu().numpy()
    assert np.all(np.isfinite(out))
    rc.assert_zero_dm_dedispersed(out, x, delays, nout)
    assert np.array_equal(out, run_block(torch, x, delays, max_delay, zero_dm=True))
    acc = torch.zeros((2, nchans), dtype=torch.float64, device="cuda")
    assert np.all(np.isfinite(engine.channel_stats_device(big[:nsamp], acc).cpu().numpy()))
    big8 = torch.full((nsamp + 300, nchans), 255, dtype=torch.uint8, device="cuda")
    big8[:nsamp] = 0
    assert not engine.zero_dm_mean_device(big8[:nsamp]).cpu().numpy().any()
    out8 = engine.dedisperse_device(big8[:nsamp], d, max_delay, zero_dm=True).cpu().numpy()
    assert out8.shape == (5, nout) and not out8.any()
    acc8 = torch.zeros((2, nchans), dtype=torch.float64, device="cuda")
    assert not engine.channel_stats_device(big8[:nsamp], acc8).cpu().numpy().any()


def test_plain_calls_unchanged(torch):
    """zero_dm=False returns the bits it returned: the same array before and
    after riptide_amd.rfi is imported, equal to the exact sums, and the _opt
    entry point with flags = 0 gives the array of the old one."""
    import importlib
    from riptide_amd import _lib, engine
    from riptide_amd.dedispersion import dedisperse, dispersion_delays
    lib = _lib.load()
    nchans, nout = 65, 500
    freqs = dc.band(nchans)
    delays, max_delay = dispersion_delays(freqs, DMS[5], dc.TSAMP)
    for dtype in DTYPES:
        x = dc.samples(np.random.RandomState(2), max_delay + nout, nchans, dtype)
        before = run_block(torch, x, delays, max_delay)
        importlib.import_module("riptide_amd.rfi")
        after = run_block(torch, x, delays, max_delay, zero_dm=False)
        assert np.array_equal(before, after)
        dc.assert_dedispersed(after, x, delays, nout)
        assert np.array_equal(dedisperse(x, freqs, dc.TSAMP, DMS[5]), after)
        block = torch.from_numpy(x).cuda()
        d = torch.from_numpy(delays.astype(np.int32)).cuda()
        ws = torch.empty(engine.dedisperse_workspace_bytes(np.dtype(dtype).name, x.shape[0], nchans), dtype=torch.uint8,
                         device="cuda")
        out = torch.empty((5, nout), dtype=torch.float32, device="cuda")
        assert lib.rt_dedisperse_device_opt(_lib.ptr(block), engine.DEDISP_DTYPES[np.dtype(dtype).name], x.shape[0],
                                            nchans, _lib.ptr(d), None, 5, max_delay, _lib.ptr(out), nout, 0,
                                            _lib.ptr(ws), ws.numel(), engine._stream_handle(), 0) == _lib.RT_OK
        assert np.array_equal(out.cpu().numpy(), after)
    # the flagged workspace is validated
    with pytest.raises(ValueError, match="workspace"):
        engine.dedisperse_device(block, d, max_delay, workspace=ws, zero_dm=True)
    with pytest.raises(ValueError, match="2\\^24"):
        engine.dedisperse_device(torch.zeros((2, 65794), dtype=torch.uint8, device="cuda"),
                                 torch.zeros((1, 65794), dtype=torch.int32, device="cuda"), 0, zero_dm=True)


def _write_filterbank(path, x, **extra):
    from riptide_amd.reading import write_sigproc
    nchans = x.shape[1]
    header = {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": dc.TSAMP,
              "nbits": 8 * x.dtype.itemsize, "fch1": 400.0, "foff": -32.0 / nchans, "nchans": nchans, "nifs": 1}
    header.update(extra)
    write_sigproc(str(path), x, header)
    return str(path)


@pytest.fixture(scope="module")
def files(torch, tmp_path_factory):
    """{dtype name: (Filterbank, samples)}: [max_delay + 2300, 37] uint8 and
    float32 files, max_delay that of DMS[5]."""
    from riptide_amd.dedispersion import dispersion_delays
    from riptide_amd.reading import Filterbank
    nchans = 37
    _, max_delay = dispersion_delays(dc.band(nchans), DMS[5], dc.TSAMP)
    d = tmp_path_factory.mktemp("rfi")
    out = {}
    for dtype in (np.uint8, np.float32):
        x = dc.samples(np.random.RandomState(6), max_delay + 2300, nchans, dtype)
        out[np.dtype(dtype).name] = (Filterbank(_write_filterbank(d / f"{np.dtype(dtype).name}.fil", x)), x)
    return out


@pytest.mark.parametrize("name", ["uint8", "float32"])
def test_zero_dm_gulp_independence(torch, files, name):
    """Gulps of max_delay + 1 samples, 777 and the whole file give the same
    bits, those of the one-block call: a sample's mean needs its row alone."""
    from riptide_amd.dedispersion import dedisperse, dedisperse_filterbank, dispersion_delays
    fb, x = files[name]
    delays, max_delay = dispersion_delays(fb.freqs, DMS[5], dc.TSAMP)
    one_block = run_block(torch, x, delays, max_delay, zero_dm=True)
    rc.assert_zero_dm_dedispersed(one_block, x, delays, x.shape[0] - max_delay)
    assert np.array_equal(dedisperse(x, fb.freqs, dc.TSAMP, DMS[5], zero_dm=True), one_block)
    mask = np.zeros(fb.nchans, dtype=bool)
    mask[5] = True
    masked = run_block(torch, x, delays, max_delay, mask=mask, zero_dm=True)
    for gulp in (max_delay + 1, 777, None):
        out = dedisperse_filterbank(fb, DMS[5], gulp=gulp, zero_dm=True)
        assert out.is_cuda and out.dtype == torch.float32
        assert np.array_equal(out.cpu().numpy(), one_block), gulp
    assert np.array_equal(dedisperse_filterbank(fb, DMS[5], mask=mask, gulp=777, zero_dm=True).cpu().numpy(), masked)
    # the plain call through the shared gulp loop is what it was
    dc.assert_dedispersed(dedisperse_filterbank(fb, DMS[5], gulp=777).cpu().numpy(), x, delays,
                          x.shape[0] - max_delay)
    # the budget counts the flagged workspace: four times the 8-bit one and the mean series
    if name == "uint8":
        ndm, nout = 5, x.shape[0] - max_delay
        budget = ndm * nout * 4 + 2 * 777 * fb.nchans + 784 * fb.nchans
        dedisperse_filterbank(fb, DMS[5], gulp=777, budget_bytes=budget)
        with pytest.raises(ValueError, match="pass fewer DMs per call"):
            dedisperse_filterbank(fb, DMS[5], gulp=777, budget_bytes=budget, zero_dm=True)


@pytest.mark.parametrize("name", ["uint8", "float32"])
def test_channel_stats(torch, files, name):
    """rfi.channel_stats at two gulps.  8-bit: numpy's int64 sums exactly.
    float32: a float64 accumulation of n terms in any order is within
    n * 2^-53 * sum |x| of the exact sum.  Twice the same bits; nsamp=
    restricts the range; zero_dm_series is the row mean of the file."""
    from riptide_amd import rfi
    fb, x = files[name]
    nsamp = x.shape[0]

    def check(stats, rows):
        xs = x[:rows]
        assert stats.nsamp == rows and stats.sum.dtype == np.float64 and stats.sum.shape == (fb.nchans,)
        if name == "uint8":
            xi = xs.astype(np.int64)
            assert np.array_equal(stats.sum, xi.sum(axis=0).astype(np.float64))
            assert np.array_equal(stats.sumsq, (xi * xi).sum(axis=0).astype(np.float64))
        else:
            x64 = xs.astype(np.float64)
            s = np.array([math.fsum(col) for col in x64.T])
            q = np.array([math.fsum(col * col) for col in x64.T])
            assert np.all(np.abs(stats.sum - s) <= rows * 2.0 ** -53 * np.abs(x64).sum(axis=0))
            assert np.all(np.abs(stats.sumsq - q) <= rows * 2.0 ** -53 * (x64 * x64).sum(axis=0))
        mean = stats.sum / rows
        assert np.array_equal(stats.mean, mean)
        assert np.array_equal(stats.std, np.sqrt(np.clip(stats.sumsq / rows - mean ** 2, 0.0, None)))
        assert np.allclose(stats.mean, xs.mean(axis=0, dtype=np.float64), rtol=1e-12)
        assert np.allclose(stats.std, xs.std(axis=0, dtype=np.float64), rtol=1e-9)

    runs = {}
    for gulp in (777, None):       # 777: three gulps, the last one short; None: one gulp of two chunks
        runs[gulp] = rfi.channel_stats(fb, gulp=gulp)
        check(runs[gulp], nsamp)
        again = rfi.channel_stats(fb, gulp=gulp)
        assert np.array_equal(again.sum, runs[gulp].sum) and np.array_equal(again.sumsq, runs[gulp].sumsq)
    check(rfi.channel_stats(fb, nsamp=1000, gulp=300), 1000)
    check(rfi.channel_stats(fb, nsamp=1), 1)
    with pytest.raises(ValueError, match="nsamp must be"):
        rfi.channel_stats(fb, nsamp=nsamp + 1)
    mask = np.zeros(fb.nchans, dtype=bool)
    mask[[0, 9]] = True
    for gulp in (777, None):
        series = rfi.zero_dm_series(fb, mask=mask, gulp=gulp)
        assert series.is_cuda and series.dtype == torch.float32
        assert np.array_equal(series.cpu().numpy(), run_mean(torch, x, mask))
    assert_mean(series.cpu().numpy(), x, mask)
    assert np.array_equal(rfi.zero_dm_series(fb, nsamp=500, gulp=128).cpu().numpy(), run_mean(torch, x[:500]))


def test_channel_stats_chunks(torch):
    """engine.channel_stats_device over several 64-channel groups and several
    chunks of time (257 channels, 5000 samples), adding into accumulators
    that are not zero; int8 squares are those of the signed values."""
    from riptide_amd import engine
    nsamp, nchans = 5000, 257
    for dtype in (np.uint8, np.int8):
        x = dc.samples(np.random.RandomState(5), nsamp, nchans, dtype)
        acc = torch.full((2, nchans), 3.0, dtype=torch.float64, device="cuda")
        ws = torch.empty(engine.channel_stats_workspace_bytes(nsamp, nchans), dtype=torch.uint8, device="cuda")
        got = engine.channel_stats_device(torch.from_numpy(x).cuda(), acc, workspace=ws)
        assert got is acc
        xi = x.astype(np.int64)
        assert np.array_equal(acc[0].cpu().numpy(), 3.0 + xi.sum(axis=0))
        assert np.array_equal(acc[1].cpu().numpy(), 3.0 + (xi * xi).sum(axis=0))
    with pytest.raises(ValueError, match="workspace"):
        engine.channel_stats_device(torch.from_numpy(x).cuda(), acc, workspace=ws[:64])
    with pytest.raises(ValueError, match="acc must be"):
        engine.channel_stats_device(torch.from_numpy(x).cuda(), acc[:, :5])


# ---------------------------------------------------------------- end to end
E2E_DMS = [0.0, 30.0]
E2E_DM, E2E_PERIOD, E2E_RFI_PERIOD = 30.0, 0.25, 0.4
E2E_STUCK = 17
E2E_DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}
E2E_RANGES = [{"name": "short",
               "ffa_search": {"period_min": 0.09, "period_max": 1.0, "bins_min": 80, "bins_max": 88},
               "find_peaks": {"smin": 7.0}}]


def _e2e_samples():
    """64 channels x 2^15 samples of 1 ms, noise N(100, 10): a train of
    8-sample pulses of amplitude 3 and period 0.25 s swept at DM 30; an
    undispersed square wave of amplitude 3, period 0.4 s and 40 samples high
    in every channel; channel 17 then stuck at 0."""
    nchans, nsamp = 64, 1 << 15
    rng = np.random.RandomState(4321)
    x = rng.normal(100.0, 10.0, size=(nsamp, nchans))
    sweep = dc.numpy_delays(dc.band(nchans), [E2E_DM], dc.TSAMP)[0]
    for c in range(nchans):
        for t0 in range(100 + int(sweep[c]), nsamp - 8, 250):
            x[t0:t0 + 8, c] += 3.0
    x[(np.arange(nsamp) % 400) < 40] += 3.0
    x[:, E2E_STUCK] = 0.0
    return np.clip(np.round(x), 0, 255).astype(np.uint8)


def _near(period, target):
    return abs(period - target) <= 0.01 * target


def test_end_to_end(torch, tmp_path):
    """Channel statistics -> mask -> search with and without the zero-DM
    filter.  The amplitudes were picked on the CPU with dedisperse_host(...,
    mask=mask, zero_dm=...) and the oracle's periodogram (dereddened and
    normalised as the searcher does), largest S/N over the widths:

      without the filter  DM 0: 104.1 at 0.4 s (64.6, 39.9, 28.3 at 0.2 s,
                                0.1333 s, 0.1 s)       DM 30: 61.7 at 0.25 s
      with the filter     DM 0: 3.9, 4.8, 4.3, 4.3 within 1 % of 0.4 s, 0.2 s,
                                0.1333 s, 0.1 s; 6.2 at most anywhere, below
                                smin = 7                DM 30: 62.3 at 0.25 s
    """
    from riptide_amd import rfi
    from riptide_amd.dispatch import EngineSearcher, search_filterbank
    from riptide_amd.reading import Filterbank
    x = _e2e_samples()
    fb = Filterbank(_write_filterbank(tmp_path / "e2e.fil", x))
    stats = rfi.channel_stats(fb)
    mask = rfi.channel_mask(stats)
    assert list(np.flatnonzero(mask)) == [E2E_STUCK]
    searcher = EngineSearcher(E2E_DEREDDEN, E2E_RANGES, device=0, batch=2)

    plain = search_filterbank(fb, E2E_DMS, searcher, mask=mask)
    dm0 = [p for p in plain if p.dm == 0.0]
    assert dm0 and _near(max(dm0, key=lambda p: p.snr).period, E2E_RFI_PERIOD)
    # without the flag the call returns what it returned: the peaks of the exact 8-bit sums
    from riptide_amd.dispatch import Trial
    delays = dc.numpy_delays(fb.freqs, E2E_DMS, fb.tsamp)
    series = dc.numpy_dedisperse(x, delays, x.shape[0] - int(delays.max()), mask)[0].astype(np.float32)
    ref = [p for plist in searcher([Trial(series[i], fb.tsamp, {"dm": dm}) for i, dm in enumerate(E2E_DMS)])
           for p in plist]
    assert [tuple(p) for p in plain] == [tuple(p) for p in ref]
    assert [tuple(p) for p in search_filterbank(fb, E2E_DMS, searcher, mask=mask, zero_dm=False)] == \
        [tuple(p) for p in plain]

    clean = search_filterbank(fb, E2E_DMS, searcher, mask=mask, zero_dm=True)
    harmonics = [E2E_RFI_PERIOD / k for k in (1, 2, 3, 4)]
    assert not [p for p in clean if p.dm == 0.0 and any(_near(p.period, h) for h in harmonics)]
    assert any(_near(p.period, E2E_PERIOD) and p.snr > 30.0 for p in clean if p.dm == E2E_DM)
