"""GPU tests of the dedispersion kernels (csrc/dedisp_kernels.hip) and the
filterbank search path built on them.  The device result is compared with the
numpy restatement of dedisp_common: bit for bit for 8-bit data; for float32
within nchans * 2^-24 * sum |x| of the float64 sums and bit for bit with the
float32 additions in channel order.  The delays come from
dispersion_delays, which test_dedisp_host.py pins to its formula."""
import os
import socket

import numpy as np
import pytest

import dedisp_common as dc

pytestmark = pytest.mark.gpu

DMS = {1: [37.0],
       5: [0.0, 50.0, 12.5, 50.0, 3.0],
       # unsorted, with DM 0 and two equal DMs; more than two DM tiles of 16
       33: list(np.random.RandomState(33).permutation(np.linspace(0.0, 50.0, 31))) + [50.0, 0.0]}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def run_block(torch, x, delays, max_delay, mask=None, **kw):
    """engine.dedisperse_device on the whole of x as one block -> numpy."""
    from riptide_amd import engine
    block = torch.from_numpy(x).cuda()
    d = torch.from_numpy(delays.astype(np.int32)).cuda()
    m = None if mask is None else torch.from_numpy(np.asarray(mask, dtype=np.uint8)).cuda()
    return engine.dedisperse_device(block, d, max_delay, mask=m, **kw).cpu().numpy()


@pytest.mark.parametrize("ndm", [1, 5, 33])
@pytest.mark.parametrize("nchans", [1, 3, 37, 64, 65, 257])
def test_channel_and_dm_tiles(torch, nchans, ndm):
    """Channel counts around the 16-channel step and the 64-channel transpose
    tile, DM counts around the 16-DM tile; 300 outputs = one full time tile
    and a partial one.  uint8 and float32."""
    from riptide_amd.dedispersion import dispersion_delays
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS[ndm], dc.TSAMP)
    rng = np.random.RandomState(nchans * 100 + ndm)
    nout = 300
    for dtype in (np.uint8, np.float32):
        x = dc.samples(rng, max_delay + nout, nchans, dtype)
        out = run_block(torch, x, delays, max_delay)
        dc.assert_dedispersed(out, x, delays, nout)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.float32])
@pytest.mark.parametrize("nout", [1, 255, 256, 257, 1000])
def test_time_tiles(torch, nout, dtype):
    """Output counts around the 256-output time tile (and 1000: no multiple of
    any tile, and a row pitch that needs padding), every sample type,
    ascending band (foff > 0)."""
    from riptide_amd.dedispersion import dispersion_delays
    nchans = 37
    delays, max_delay = dispersion_delays(dc.band(nchans, ascending=True), DMS[5], dc.TSAMP)
    x = dc.samples(np.random.RandomState(nout), max_delay + nout, nchans, dtype)
    out = run_block(torch, x, delays, max_delay)
    assert out.shape == (5, nout)
    dc.assert_dedispersed(out, x, delays, nout)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.float32])
def test_delay_spread_wider_than_the_tile(torch, dtype):
    """DMs 0 and 250 in one DM tile: their delays differ by up to ~1150
    samples, more than the 256-output time tile and more than the staged span
    holds, so the low channels are read from the workspace rows directly and
    the high channels from LDS."""
    from riptide_amd.dedispersion import dispersion_delays
    nchans = 40
    delays, max_delay = dispersion_delays(dc.band(nchans), [0.0, 250.0, 3.0, 100.0], dc.TSAMP)
    assert max_delay > 1100
    nout = 700
    x = dc.samples(np.random.RandomState(9), max_delay + nout, nchans, dtype)
    out = run_block(torch, x, delays, max_delay)
    dc.assert_dedispersed(out, x, delays, nout)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.float32])
def test_masks(torch, dtype):
    """The first channel, the last channel, both, and every channel but one
    zapped: the zapped channels are skipped, the alignment is unchanged."""
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
        out = run_block(torch, x, delays, max_delay, mask=mask)
        dc.assert_dedispersed(out, x, delays, nout, mask)


def test_largest_exact_sum(torch):
    """4096 channels of 255: every sum is 1044480, exactly."""
    from riptide_amd.dedispersion import dedisperse
    nchans = 4096
    x = np.full((560, nchans), 255, dtype=np.uint8)
    out = dedisperse(x, dc.band(nchans), dc.TSAMP, [0.0, 50.0, 20.0])
    assert out.shape[0] == 3 and 300 < out.shape[1] < 340
    assert np.all(out == np.float32(255 * 4096))


def test_host_buffer_form_and_output_window(torch):
    """rt_dedisperse equals the block call; out_offset / a wider out leave
    everything outside the block's window untouched."""
    from riptide_amd.dedispersion import dedisperse, dispersion_delays
    nchans, nout = 65, 500
    freqs = dc.band(nchans)
    delays, max_delay = dispersion_delays(freqs, DMS[5], dc.TSAMP)
    x = dc.samples(np.random.RandomState(2), max_delay + nout, nchans, np.int8)
    out = dedisperse(x, freqs, dc.TSAMP, DMS[5])
    dc.assert_dedispersed(out, x, delays, nout)
    wide = torch.full((5, nout + 40), -7.0, dtype=torch.float32, device="cuda")
    got = run_block(torch, x, delays, max_delay, out=wide, out_offset=13)
    assert np.array_equal(got[:, 13:13 + nout], out)
    assert np.all(got[:, :13] == -7.0) and np.all(got[:, 13 + nout:] == -7.0)


def test_no_over_read(torch):
    """The block is the first nsamp_blk rows of a larger allocation whose
    remainder is poison (NaN for float32; 255 under an all-zero block for
    uint8): nothing of it reaches the output."""
    from riptide_amd import engine
    from riptide_amd.dedispersion import dispersion_delays
    nchans, nout = 37, 257
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS[5], dc.TSAMP)
    nsamp = max_delay + nout
    d = torch.from_numpy(delays.astype(np.int32)).cuda()
    x = dc.samples(np.random.RandomState(8), nsamp, nchans, np.float32)
    big = torch.full((nsamp + 300, nchans), float("nan"), dtype=torch.float32, device="cuda")
    big[:nsamp] = torch.from_numpy(x).cuda()
    out = engine.dedisperse_device(big[:nsamp], d, max_delay).cpu().numpy()
    assert np.all(np.isfinite(out))
    dc.assert_dedispersed(out, x, delays, nout)
    assert np.array_equal(out, run_block(torch, x, delays, max_delay))
    big8 = torch.full((nsamp + 300, nchans), 255, dtype=torch.uint8, device="cuda")
    big8[:nsamp] = 0
    out8 = engine.dedisperse_device(big8[:nsamp], d, max_delay).cpu().numpy()
    assert out8.shape == (5, nout) and not out8.any()


def _write_filterbank(path, x, foff=-1.0, **extra):
    from riptide_amd.reading import write_sigproc
    nchans = x.shape[1]
    step = 32.0 / nchans
    header = {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": dc.TSAMP,
              "nbits": 8 * x.dtype.itemsize, "fch1": 400.0 if foff < 0 else 368.0,
              "foff": -step if foff < 0 else step, "nchans": nchans, "nifs": 1}
    header.update(extra)
    write_sigproc(str(path), x, header)
    return str(path)


@pytest.mark.parametrize("dtype,extra", [(np.uint8, {}), (np.int8, {"signed": True}), (np.float32, {})])
def test_gulp_independence(torch, tmp_path, dtype, extra):
    """Gulps of max_delay + 1 samples (one output each), a prime, and the
    whole file give the same tensor, equal to dedisperse() of the host array."""
    from riptide_amd.dedispersion import dedisperse, dedisperse_filterbank, dispersion_delays
    from riptide_amd.reading import Filterbank
    nchans, nsamp = 37, 1500
    x = dc.samples(np.random.RandomState(6), nsamp, nchans, dtype)
    fb = Filterbank(_write_filterbank(tmp_path / "g.fil", x, **extra))
    assert np.array_equal(fb.freqs, dc.band(nchans))
    delays, max_delay = dispersion_delays(fb.freqs, DMS[5], dc.TSAMP)
    host = dedisperse(x, fb.freqs, dc.TSAMP, DMS[5])
    dc.assert_dedispersed(host, x, delays, nsamp - max_delay)
    mask = np.zeros(nchans, dtype=bool)
    mask[5] = True
    host_masked = dedisperse(x, fb.freqs, dc.TSAMP, DMS[5], mask=mask)
    for gulp in (max_delay + 1, 1009, nsamp, None):
        out = dedisperse_filterbank(fb, DMS[5], gulp=gulp)
        assert out.is_cuda and out.dtype == torch.float32
        assert np.array_equal(out.cpu().numpy(), host), gulp
    assert np.array_equal(dedisperse_filterbank(fb, DMS[5], mask=mask, gulp=1009).cpu().numpy(), host_masked)
    cut = dedisperse_filterbank(fb, DMS[5], gulp=1009, nout=777)
    assert np.array_equal(cut.cpu().numpy(), host[:, :777])


def test_chained_calls_without_host_wait(torch, tmp_path):
    """Two calls back to back, nothing waiting for the device in between: the
    second call's buffers may be the first call's, still being read by its
    last kernels, so its uploads must be ordered behind them."""
    from riptide_amd.dedispersion import dedisperse, dedisperse_filterbank
    from riptide_amd.reading import Filterbank
    nchans, nsamp = 64, 6000
    rng = np.random.RandomState(12)
    xa, xb = (dc.samples(rng, nsamp, nchans, np.uint8) for _ in range(2))
    fa = Filterbank(_write_filterbank(tmp_path / "a.fil", xa))
    fb = Filterbank(_write_filterbank(tmp_path / "b.fil", xb))
    outs = []
    for _ in range(3):
        outs.append((dedisperse_filterbank(fa, DMS[33], gulp=2048), dedisperse_filterbank(fb, DMS[33], gulp=2048)))
    ra, rb = dedisperse(xa, fa.freqs, dc.TSAMP, DMS[33]), dedisperse(xb, fb.freqs, dc.TSAMP, DMS[33])
    for oa, ob in outs:
        assert np.array_equal(oa.cpu().numpy(), ra) and np.array_equal(ob.cpu().numpy(), rb)


def test_errors(torch, tmp_path):
    from riptide_amd import engine
    from riptide_amd.dedispersion import dedisperse, dedisperse_filterbank
    from riptide_amd.reading import Filterbank
    x = np.zeros((1500, 8), dtype=np.uint8)
    fb = Filterbank(_write_filterbank(tmp_path / "e.fil", x))
    with pytest.raises(ValueError, match="pass fewer DMs per call"):
        dedisperse_filterbank(fb, DMS[5], budget_bytes=20000)
    with pytest.raises(ValueError, match="largest delay"):
        dedisperse_filterbank(fb, [400.0])
    with pytest.raises(ValueError, match="largest delay"):
        dedisperse(x[:100], fb.freqs, dc.TSAMP, [50.0])
    with pytest.raises(ValueError, match="gulp must exceed"):
        dedisperse_filterbank(fb, [50.0], gulp=10)
    wide = np.zeros((2, 65794), dtype=np.uint8)
    with pytest.raises(ValueError, match="65793"):
        dedisperse(wide, np.linspace(400.0, 368.0, 65794), dc.TSAMP, [0.0])
    with pytest.raises(ValueError, match="2\\^24"):
        engine.dedisperse_device(torch.zeros((2, 65794), dtype=torch.uint8, device="cuda"),
                                 torch.zeros((1, 65794), dtype=torch.int32, device="cuda"), 0)
    block = torch.zeros((100, 8), dtype=torch.uint8, device="cuda")
    d = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="max_delay"):
        engine.dedisperse_device(block, d, 100)
    with pytest.raises(ValueError, match="workspace"):
        engine.dedisperse_device(block, d, 0, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        engine.dedisperse_device(block, d, 0, out=torch.zeros((1, 50), dtype=torch.float32, device="cuda"))


# ---------------------------------------------------------------- end to end
E2E_DMS = [0.0, 5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 35.0, 40.0]
E2E_DM, E2E_PERIOD = 20.0, 0.5
E2E_DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}
E2E_RANGES = [{"name": "short",
               "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
               "find_peaks": {"smin": 7.0}}]


def _e2e_filterbank(path):
    """32 channels x 2^16 samples of 1 ms: a train of 8-sample pulses of
    period 0.5 s, swept at DM 20, over seeded noise."""
    nchans, nsamp = 32, 1 << 16
    rng = np.random.RandomState(1234)
    x = rng.normal(100.0, 10.0, size=(nsamp, nchans))
    sweep = dc.numpy_delays(dc.band(nchans), [E2E_DM], dc.TSAMP)[0]
    period = int(round(E2E_PERIOD / dc.TSAMP))
    for c in range(nchans):
        for t0 in range(100 + int(sweep[c]), nsamp - 8, period):
            x[t0:t0 + 8, c] += 4.0
    return _write_filterbank(path, np.clip(np.round(x), 0, 255).astype(np.uint8)), nsamp


@pytest.fixture(scope="module")
def e2e(torch, tmp_path_factory):
    """(file name, peaks of search_filterbank, peaks of the host path): the
    same nine series, dedispersed by numpy, searched as Trials."""
    from riptide_amd.dispatch import EngineSearcher, Trial, search_filterbank
    from riptide_amd.reading import Filterbank
    fname, nsamp = _e2e_filterbank(tmp_path_factory.mktemp("fb") / "e2e.fil")
    fb = Filterbank(fname)
    searcher = EngineSearcher(E2E_DEREDDEN, E2E_RANGES, device=0, batch=4)
    got = search_filterbank(fb, E2E_DMS, searcher)
    delays = dc.numpy_delays(fb.freqs, E2E_DMS, fb.tsamp)
    nout = nsamp - int(delays.max())
    series = dc.numpy_dedisperse(np.asarray(fb.data), delays, nout)[0].astype(np.float32)
    trials = [Trial(series[i], fb.tsamp, {"dm": dm}) for i, dm in enumerate(E2E_DMS)]
    ref = [p for plist in searcher(trials) for p in plist]
    return fname, got, ref


def test_search_filterbank_equals_the_host_path(e2e):
    """The series are bit-identical, so the peak lists are equal; the
    highest-S/N peak is at the injected DM and period.  Period tolerance: two
    steps of the trial grid, a step being at most the drift of one phase bin
    over the observation, p * (p / bins_min) / tobs."""
    _, got, ref = e2e
    assert len(got) > 0
    assert [tuple(p) for p in got] == [tuple(p) for p in ref]
    dms = [p.dm for p in got]
    assert dms == sorted(dms) and set(dms) <= set(E2E_DMS)      # in the order of the DM list
    best = max(got, key=lambda p: p.snr)
    assert best.dm == E2E_DM
    step = E2E_PERIOD * (E2E_PERIOD / 240) / (65536 * dc.TSAMP)
    assert abs(best.period - E2E_PERIOD) <= 2 * step, best


def test_search_filterbank_other_dispersion_constant(e2e):
    """kdm reaches the delay table of the search path: three DMs at a constant
    8 % above the default (far enough to move the delays by whole samples)
    give the peaks of the series numpy dedisperses with it."""
    from riptide_amd.dispatch import EngineSearcher, Trial, search_filterbank
    from riptide_amd.reading import Filterbank
    fb = Filterbank(e2e[0])
    kdm, dms = 4.5e3, [15.0, 20.0, 40.0]
    searcher = EngineSearcher(E2E_DEREDDEN, E2E_RANGES, device=0, batch=2)
    got = search_filterbank(fb, dms, searcher, kdm=kdm)
    delays = dc.numpy_delays(fb.freqs, dms, fb.tsamp, kdm)
    assert delays.max() != dc.numpy_delays(fb.freqs, dms, fb.tsamp).max()
    series = dc.numpy_dedisperse(np.asarray(fb.data), delays, fb.nsamp - int(delays.max()))[0].astype(np.float32)
    ref = [p for plist in searcher([Trial(series[i], fb.tsamp, {"dm": dm}) for i, dm in enumerate(dms)])
           for p in plist]
    assert len(got) > 0 and [tuple(p) for p in got] == [tuple(p) for p in ref]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _filterbank_worker(rank, world, port, fname, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import riptide_amd
        from riptide_amd.dispatch import EngineSearcher
        peaks = riptide_amd.search_filterbank(fname, E2E_DMS, EngineSearcher(E2E_DEREDDEN, E2E_RANGES, device=0,
                                                                             batch=4))
        q.put((rank, [tuple(p) for p in peaks]))
    except Exception as e:  # reported to the parent
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_search_filterbank_two_ranks(e2e):
    """Two gloo ranks driving cuda:0: each dedisperses and searches its
    round-robin share of the DMs; both gather the single-process list."""
    import torch.multiprocessing as mp
    fname, got, _ = e2e
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_filterbank_worker, args=(r, 2, port, fname, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=100) for _ in procs)
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    assert not isinstance(results[0], str), results[0]
    assert not isinstance(results[1], str), results[1]
    assert results[0] == results[1] == [tuple(p) for p in got]
