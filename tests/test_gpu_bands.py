"""GPU tests of sub-band dedispersion (dedisp_sum_kernel<T, DdBandTable> in
csrc/dedisp_kernels.hip) and of what is built on it: dedisperse_filterbank
with bands, band_series and build_candidates_filterbank.  The device result is
compared with the host specification rt_dedisperse_bands_host, which
test_bands_host.py pins to the numpy restatement: bit for bit for integer
data, within (band width) * 2^-24 * sum |x| of the float64 sums for float32."""
import numpy as np
import pytest

import dedisp_common as dc
from dered_common import NORM_BOUND
from test_bands_host import BANDS, assert_band_rows
from test_gpu_dedisp import DMS, _write_filterbank
from test_lowbit_host import write_packed

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.float32]
EMPTY = 8    # BANDS[EMPTY] is [9, 9)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def run_bands(torch, x, delays, max_delay, bands, mask=None, **kw):
    """engine.dedisperse_bands_device on the whole of x as one block -> numpy."""
    from riptide_amd import engine
    block = torch.from_numpy(x).cuda()
    d = torch.from_numpy(delays.astype(np.int32)).cuda()
    m = None if mask is None else torch.from_numpy(np.asarray(mask, dtype=np.uint8)).cuda()
    return engine.dedisperse_bands_device(block, d, max_delay, bands, mask=m, **kw).cpu().numpy()


def run_plain(torch, x, delays, max_delay, mask=None, **kw):
    from riptide_amd import engine
    block = torch.from_numpy(x).cuda()
    d = torch.from_numpy(delays.astype(np.int32)).cuda()
    m = None if mask is None else torch.from_numpy(np.asarray(mask, dtype=np.uint8)).cuda()
    return engine.dedisperse_device(block, d, max_delay, mask=m, **kw).cpu().numpy()


def check(out, x, delays, max_delay, nout, bands, mask=None):
    """Integer data: the host specification's bits.  float32: the bound against
    the float64 sums (and the host specification is inside it too), and the
    bits of dc.numpy_dedisperse_f32 -- the float32 additions in ascending
    channel order within each band -- which are the host specification's."""
    from riptide_amd.dedispersion import dedisperse_bands_host
    host = dedisperse_bands_host(x, delays, max_delay, bands, mask=mask, nout=nout)
    if x.dtype == np.float32:
        assert_band_rows(out, x, delays, nout, bands, mask)
        assert_band_rows(host, x, delays, nout, bands, mask)
        ref = dc.numpy_dedisperse_f32(x, delays, nout, mask, bands=bands)
        dc.assert_same_bits(host, ref, "host specification, float32 sums in channel order")
        dc.assert_same_bits(out, ref, "float32 sums in channel order")
    else:
        assert out.dtype == np.float32 and np.array_equal(out, host), \
            f"{int((out != host).sum())} of {out.size} sums differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ndm", [1, 5, 33])
def test_band_edges_around_the_channel_step(torch, ndm, dtype):
    """37 channels, band edges on, before and after the 16-channel step,
    overlapping, one band empty, the table unsorted; DM counts around the
    16-DM tile; 300 outputs = a full time tile and a partial one."""
    from riptide_amd.dedispersion import dispersion_delays
    nchans, nout = 37, 300
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS[ndm], dc.TSAMP)
    x = dc.samples(np.random.RandomState(ndm), max_delay + nout, nchans, dtype)
    out = run_bands(torch, x, delays, max_delay, BANDS)
    assert out.shape == (ndm, len(BANDS), nout)
    check(out, x, delays, max_delay, nout, BANDS)
    assert not out[:, EMPTY].any()


def test_masked_bands(torch):
    """int8, where a wrong channel count shows as a multiple of the bias 128:
    a mask that zaps one whole band, the first channel of another and the last
    channel of a third.  The all-masked band is exactly zero."""
    from riptide_amd.dedispersion import dispersion_delays
    nchans, nout = 37, 300
    bands = np.array([[0, 8], [8, 20], [20, 30], [30, 37], [0, 37], [8, 22]], dtype=np.uint32)
    mask = np.zeros(nchans, dtype=bool)
    mask[8:20] = True
    mask[20] = mask[36] = True
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS[5], dc.TSAMP)
    x = dc.samples(np.random.RandomState(3), max_delay + nout, nchans, np.int8)
    out = run_bands(torch, x, delays, max_delay, bands, mask=mask)
    check(out, x, delays, max_delay, nout, bands, mask)
    assert not out[:, 1].any() and out[:, 0].any() and out[:, 5].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nout", [1, 255, 256, 257])
def test_time_tiles(torch, nout, dtype):
    """Output counts around the 256-output time tile, ascending band."""
    from riptide_amd.dedispersion import dispersion_delays
    nchans = 37
    delays, max_delay = dispersion_delays(dc.band(nchans, ascending=True), DMS[5], dc.TSAMP)
    x = dc.samples(np.random.RandomState(nout), max_delay + nout, nchans, dtype)
    out = run_bands(torch, x, delays, max_delay, BANDS)
    assert out.shape == (5, len(BANDS), nout)
    check(out, x, delays, max_delay, nout, BANDS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_delay_spread_wider_than_the_tile(torch, dtype):
    """DMs 0 and 250 in one DM tile (test_gpu_dedisp.py's case): the low
    channels are read from the workspace rows directly, the high ones from
    LDS, and bands lie in either part and across both."""
    from riptide_amd.dedispersion import dispersion_delays
    nchans, nout = 40, 700
    delays, max_delay = dispersion_delays(dc.band(nchans), [0.0, 250.0, 3.0, 100.0], dc.TSAMP)
    assert max_delay > 1100
    bands = np.array([[0, 40], [0, 13], [13, 27], [27, 40], [5, 35], [39, 40]], dtype=np.uint32)
    x = dc.samples(np.random.RandomState(9), max_delay + nout, nchans, dtype)
    out = run_bands(torch, x, delays, max_delay, bands)
    check(out, x, delays, max_delay, nout, bands)


@pytest.mark.parametrize("zero_dm", [False, True])
@pytest.mark.parametrize("kind", ["uint8", "int8", "float32", "u2", "u16"])
def test_full_band_equals_the_plain_call(torch, kind, zero_dm):
    """The row of the band [0, nchans) has the bits of engine.dedisperse_device
    for every sample type, float sums and the zero-DM filter included: the same
    additions in the same order.  For uint8 the rows of a partition add up to
    the plain row exactly."""
    from riptide_amd.dedispersion import band_edges, dedisperse_bands_host, dispersion_delays, zero_dm_mean_host
    from riptide_amd.reading import pack_samples, unpack_samples
    nchans, nout = 36, 300
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS[5], dc.TSAMP)
    rng = np.random.RandomState(11)
    nbits = None
    if kind in ("u2", "u16"):
        nbits = int(kind[1:])
        x = pack_samples(rng.randint(0, 1 << nbits, size=(max_delay + nout, nchans)), nbits)
    else:
        x = dc.samples(rng, max_delay + nout, nchans, kind)
    mask = np.zeros(nchans, dtype=bool)
    mask[17] = True
    bands = np.concatenate([band_edges(nchans, 5), np.array([[0, nchans]], dtype=np.uint32)])
    for m in (None, mask):
        out = run_bands(torch, x, delays, max_delay, bands, mask=m, zero_dm=zero_dm, nbits=nbits)
        plain = run_plain(torch, x, delays, max_delay, mask=m, zero_dm=zero_dm, nbits=nbits)
        assert np.array_equal(out[:, -1], plain)
        if kind == "uint8" and not zero_dm:
            assert np.array_equal(out[:, :-1].sum(axis=1, dtype=np.float64), plain.astype(np.float64))
        host = dedisperse_bands_host(x, delays, max_delay, bands, mask=m, nout=nout, zero_dm=zero_dm, nbits=nbits)
        if zero_dm or kind in ("float32", "u16"):
            # float32 sums: both inside the bound of the float64 sums of the same rows
            vals = x if nbits is None else unpack_samples(x, nbits, nchans)
            rows = vals.astype(np.float32)
            if zero_dm:
                rows = rows - zero_dm_mean_host(x, mask=m, nbits=nbits)[:, None]
            assert_band_rows(out, rows, delays, nout, bands, m)
            assert_band_rows(host, rows, delays, nout, bands, m)
        else:
            assert np.array_equal(out, host)


KINDS = ["uint8", "int8", "float32", "u1", "u2", "u4", "u16"]


@pytest.mark.parametrize("zero_dm", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_every_sample_type_with_bands(torch, kind, zero_dm):
    """Every sample type x the zero-DM filter through the band call, against
    dedisperse_bands_host by test_full_band_equals_the_plain_call's comparison:
    the host's bits for integer sums, both inside the float64 bound for float32
    sums.  40 channels: 1-bit rows of 5 bytes (byte loads), 4-bit rows of 20
    (dword loads), two 16-channel steps and a tail of 8; 17 DMs and 257 outputs:
    one live row in the second DM tile, one sample in the second time tile; one
    channel masked.  The row of [0, 40) has the plain call's bits and the empty
    band is zero."""
    from riptide_amd.dedispersion import dedisperse_bands_host, dispersion_delays, zero_dm_mean_host
    from riptide_amd.reading import pack_samples, unpack_samples
    nchans, ndm, nout = 40, 17, 257
    bands = np.array([[0, 40], [5, 21], [16, 16], [33, 40]], dtype=np.uint32)
    delays, max_delay = dispersion_delays(dc.band(nchans), np.linspace(0.0, 8.0, ndm), dc.TSAMP)
    assert 20 <= max_delay <= 60
    rng = np.random.RandomState(KINDS.index(kind))
    nbits = int(kind[1:]) if kind in ("u1", "u2", "u4", "u16") else None
    if nbits:
        x = pack_samples(rng.randint(0, 1 << nbits, size=(max_delay + nout, nchans)), nbits)
        assert x.shape[1] == nchans * nbits // 8
    else:
        x = dc.samples(rng, max_delay + nout, nchans, kind)
    mask = np.zeros(nchans, dtype=bool)
    mask[18] = True
    out = run_bands(torch, x, delays, max_delay, bands, mask=mask, zero_dm=zero_dm, nbits=nbits)
    host = dedisperse_bands_host(x, delays, max_delay, bands, mask=mask, nout=nout, zero_dm=zero_dm, nbits=nbits)
    assert out.shape == host.shape == (ndm, len(bands), nout)
    if zero_dm or kind in ("float32", "u16"):
        vals = x if nbits is None else unpack_samples(x, nbits, nchans)
        rows = vals.astype(np.float32)
        if zero_dm:
            rows = rows - zero_dm_mean_host(x, mask=mask, nbits=nbits)[:, None]
        assert_band_rows(out, rows, delays, nout, bands, mask)
        assert_band_rows(host, rows, delays, nout, bands, mask)
    else:
        assert np.array_equal(out, host)
    assert np.array_equal(out[:, 0], run_plain(torch, x, delays, max_delay, mask=mask, zero_dm=zero_dm, nbits=nbits))
    assert not out[:, 2].any() and out[:, 3].any()


def test_output_window(torch):
    """test_gpu_dedisp.py's window case: the host-buffer form equals the block
    call, out_offset is honoured and a sentinel outside the window survives."""
    from riptide_amd.dedispersion import dedisperse_bands, dispersion_delays
    nchans, nout = 65, 500
    freqs = dc.band(nchans)
    bands = np.array([[0, 65], [0, 16], [16, 64], [64, 65], [30, 30]], dtype=np.uint32)
    delays, max_delay = dispersion_delays(freqs, DMS[5], dc.TSAMP)
    x = dc.samples(np.random.RandomState(2), max_delay + nout, nchans, np.int8)
    out = dedisperse_bands(x, freqs, dc.TSAMP, DMS[5], bands)
    check(out, x, delays, max_delay, nout, bands)
    wide = torch.full((5, len(bands), nout + 40), -7.0, dtype=torch.float32, device="cuda")
    got = run_bands(torch, x, delays, max_delay, bands, out=wide, out_offset=13)
    assert np.array_equal(got[:, :, 13:13 + nout], out)
    assert np.all(got[:, :, :13] == -7.0) and np.all(got[:, :, 13 + nout:] == -7.0)


def test_no_over_read(torch):
    """test_gpu_dedisp.py's poison case: the block is the first rows of a
    larger allocation whose remainder is NaN (float32) or 255 under an
    all-zero block (uint8); nothing of it reaches any band."""
    from riptide_amd import engine
    from riptide_amd.dedispersion import dispersion_delays
    nchans, nout = 37, 257
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS[5], dc.TSAMP)
    nsamp = max_delay + nout
    d = torch.from_numpy(delays.astype(np.int32)).cuda()
    x = dc.samples(np.random.RandomState(8), nsamp, nchans, np.float32)
    big = torch.full((nsamp + 300, nchans), float("nan"), dtype=torch.float32, device="cuda")
    big[:nsamp] = torch.from_numpy(x).cuda()
    out = engine.dedisperse_bands_device(big[:nsamp], d, max_delay, BANDS).cpu().numpy()
    assert np.all(np.isfinite(out))
    check(out, x, delays, max_delay, nout, BANDS)
    assert np.array_equal(out, run_bands(torch, x, delays, max_delay, BANDS))
    big8 = torch.full((nsamp + 300, nchans), 255, dtype=torch.uint8, device="cuda")
    big8[:nsamp] = 0
    out8 = engine.dedisperse_bands_device(big8[:nsamp], d, max_delay, BANDS).cpu().numpy()
    assert out8.shape == (5, len(BANDS), nout) and not out8.any()


def test_device_errors(torch):
    from riptide_amd import engine
    block = torch.zeros((100, 8), dtype=torch.uint8, device="cuda")
    d = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    ok = np.array([[0, 4], [4, 8]], dtype=np.uint32)
    assert engine.dedisperse_bands_device(block, d, 0, ok).shape == (1, 2, 100)
    with pytest.raises(ValueError, match="nbands must be at least 1"):
        engine.dedisperse_bands_device(block, d, 0, np.zeros((0, 2), dtype=np.uint32))
    with pytest.raises(ValueError, match="too many bands"):
        engine.dedisperse_bands_device(block, d, 0, torch.zeros((65536, 2), dtype=torch.int32, device="cuda"),
                                       out=torch.zeros((1, 65536, 100), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="lo <= hi <= 8"):
        engine.dedisperse_bands_device(block, d, 0, [[0, 9]])
    with pytest.raises(ValueError, match="lo <= hi <= 8"):
        engine.dedisperse_bands_device(block, d, 0, [[5, 4]])
    with pytest.raises(ValueError, match="max_delay"):
        engine.dedisperse_bands_device(block, d, 100, ok)
    with pytest.raises(ValueError, match="workspace"):
        engine.dedisperse_bands_device(block, d, 0, ok, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        engine.dedisperse_bands_device(block, d, 0, ok, out=torch.zeros((1, 2, 50), dtype=torch.float32,
                                                                        device="cuda"))
    # a table already on the device is not validated on the host: its edges are clamped as they are read
    wild = torch.tensor([[0, 1000], [7, 3], [6, 8]], dtype=torch.int32, device="cuda")
    ones = torch.ones((100, 8), dtype=torch.uint8, device="cuda")
    got = engine.dedisperse_bands_device(ones, d, 0, wild).cpu().numpy()
    assert np.all(got[0, 0] == 8.0) and not got[0, 1].any() and np.all(got[0, 2] == 2.0)


@pytest.mark.parametrize("kind", ["u2", "float32"])
def test_gulp_independence(torch, tmp_path, kind):
    """dedisperse_filterbank(bands=...) of a written file: a gulp of
    max_delay + 1 samples, a prime and the whole file give the same tensor,
    the host-buffer form's."""
    from riptide_amd.dedispersion import dedisperse_bands, dedisperse_filterbank, dispersion_delays
    from riptide_amd.reading import open_filterbank, pack_samples
    nchans, nsamp = 36, 1500
    rng = np.random.RandomState(6)
    bands = np.minimum(BANDS, nchans)
    if kind == "u2":
        x = rng.randint(0, 4, size=(nsamp, nchans)).astype(np.uint8)
        fb = open_filterbank(write_packed(tmp_path / "g.fil", x, 2))
        data, nbits = pack_samples(x, 2), 2
    else:
        x = dc.samples(rng, nsamp, nchans, np.float32)
        fb = open_filterbank(_write_filterbank(tmp_path / "g.fil", x))
        data, nbits = x, None
    delays, max_delay = dispersion_delays(fb.freqs, DMS[5], dc.TSAMP)
    nout = nsamp - max_delay
    mask = np.zeros(nchans, dtype=bool)
    mask[5] = True
    for m, zero_dm in ((None, False), (mask, False), (None, True)):
        host = dedisperse_bands(data, fb.freqs, dc.TSAMP, DMS[5], bands, mask=m, zero_dm=zero_dm, nbits=nbits)
        assert host.shape == (5, len(bands), nout)
        if not zero_dm:
            check(host, data if nbits is None else x, delays, max_delay, nout, bands, m)
        for gulp in (max_delay + 1, 1009, nsamp):
            out = dedisperse_filterbank(fb, DMS[5], mask=m, gulp=gulp, zero_dm=zero_dm, bands=bands)
            assert out.is_cuda and out.dtype == torch.float32
            assert np.array_equal(out.cpu().numpy(), host), (gulp, zero_dm)
    cut = dedisperse_filterbank(fb, DMS[5], gulp=1009, nout=777, bands=bands)
    assert np.array_equal(cut.cpu().numpy(), dedisperse_bands(data, fb.freqs, dc.TSAMP, DMS[5], bands,
                                                              nbits=nbits)[:, :, :777])
    # the budget counts every band's rows: one byte short of them plus the gulp buffers
    from riptide_amd import engine
    fixed = 2 * nsamp * fb.data.shape[1] * fb.data.itemsize + engine.dedisperse_workspace_bytes(
        fb.data.dtype.name, nsamp, nchans, nbits=nbits)
    budget = fixed + 5 * len(bands) * nout * 4 - 1
    with pytest.raises(ValueError, match="pass fewer DMs per call"):
        dedisperse_filterbank(fb, DMS[5], bands=bands, budget_bytes=budget)
    assert dedisperse_filterbank(fb, DMS[5], budget_bytes=budget).shape == (5, nout)     # the plain call fits
    assert dedisperse_filterbank(fb, DMS[5], bands=bands, budget_bytes=budget + 1).shape == (5, len(bands), nout)


DEREDDEN = {"rmed_width": 0.5, "rmed_minpts": 101}


def test_band_series(torch, tmp_path):
    """The raw sums are dedisperse_filterbank(bands=...)'s, pinned to the
    host specification; every row is then what TimeSeries.deredden().normalise()
    makes of it, within dered_common's NORM_BOUND; a band whose channels are
    all masked stays zero and is flagged."""
    from riptide_amd import TimeSeries
    from riptide_amd.dedispersion import band_edges, band_series, dedisperse_filterbank, dispersion_delays
    from riptide_amd.reading import open_filterbank
    nchans, nsamp, dms = 37, 4000, [0.0, 50.0, 12.5]
    x = dc.samples(np.random.RandomState(21), nsamp, nchans, np.uint8)
    fb = open_filterbank(_write_filterbank(tmp_path / "s.fil", x))
    bands = np.concatenate([band_edges(nchans, 4), np.array([[0, nchans]], dtype=np.uint32)])
    mask = np.zeros(nchans, dtype=bool)
    mask[bands[1, 0]:bands[1, 1]] = True
    mask[30] = True
    delays, max_delay = dispersion_delays(fb.freqs, dms, dc.TSAMP)
    nout = nsamp - max_delay - 100
    raw = dedisperse_filterbank(fb, dms, mask=mask, nout=nout, bands=bands).cpu().numpy()
    check(raw, x, delays, max_delay, nout, bands, mask)
    series, empty = band_series(fb, dms, bands, DEREDDEN, nout, mask=mask)
    assert series.is_cuda and tuple(series.shape) == (3, 5, nout)
    assert empty.dtype == bool and list(empty) == [False, True, False, False, False]
    got = series.cpu().numpy()
    assert not got[:, 1].any()
    for d in range(3):
        for b in (0, 2, 3, 4):
            ref = TimeSeries.from_numpy_array(raw[d, b], dc.TSAMP).deredden(
                DEREDDEN["rmed_width"], minpts=DEREDDEN["rmed_minpts"]).normalise().data
            err = np.abs(got[d, b].astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)
            assert err.max() <= NORM_BOUND, (d, b, err.max())
    # no mask: no gather of rows; the band the mask left whole has the same raw sums
    plain, none = band_series(fb, dms, bands, DEREDDEN, nout)
    assert not none.any()
    err = np.abs(plain.cpu().numpy()[:, 0].astype(np.float64) - got[:, 0]) / np.maximum(np.abs(got[:, 0]), 1.0)
    assert err.max() <= 2 * NORM_BOUND       # both within NORM_BOUND of the same reference


# ------------------------------------------------------------- candidates
CAND_PERIOD, CAND_DM, CAND_NSUB = 0.5, 20.0, 4
CAND_RANGES = [{"name": "short",
                "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
                "candidates": {"bins": 64, "subints": 4}}]


def _candidate_filterbank(path):
    """32 channels x 8192 samples of 1 ms, 16 periods: 8-sample pulses of
    period 0.5 s, swept at DM 20, over seeded noise (test_gpu_dedisp.py's
    _e2e_filterbank, an eighth as long and the pulse three times as high, so
    that a quarter of the band shows it)."""
    nchans, nsamp = 32, 8192
    rng = np.random.RandomState(1234)
    x = rng.normal(100.0, 10.0, size=(nsamp, nchans))
    sweep = dc.numpy_delays(dc.band(nchans), [CAND_DM], dc.TSAMP)[0]
    period = int(round(CAND_PERIOD / dc.TSAMP))
    for c in range(nchans):
        for t0 in range(100 + int(sweep[c]), nsamp - 8, period):
            x[t0:t0 + 8, c] += 12.0
    return _write_filterbank(path, np.clip(np.round(x), 0, 255).astype(np.uint8))


def test_build_candidates_filterbank(torch, tmp_path, monkeypatch):
    import pandas  # noqa: F401  (Candidate.peaks is a DataFrame)
    from riptide_amd import Peak, PeakCluster, build_candidates_filterbank, dedispersion, engine
    from riptide_amd.dedispersion import band_edges, band_series, dispersion_delays
    passes = []      # the DMs of every pass over the file

    def counted(fb, dms, *args, **kw):
        passes.append(list(dms))
        return band_series(fb, dms, *args, **kw)
    monkeypatch.setattr(dedispersion, "band_series", counted)
    from riptide_amd.reading import open_filterbank
    fname = _candidate_filterbank(tmp_path / "c.fil")
    fb = open_filterbank(fname)

    def peak(period, snr, dm, width=3):
        return Peak(period=period, freq=1.0 / period, width=width, ducy=width / 64, iw=1, ip=0, snr=snr, dm=dm)

    clusters = [
        PeakCluster([peak(CAND_PERIOD, 12.0, 0.0)], rank=2),
        PeakCluster([peak(CAND_PERIOD, 30.0, CAND_DM), peak(0.5001, 11.0, 0.0)], rank=0),
        PeakCluster([peak(20.0, 25.0, CAND_DM)], rank=1),              # longer than the data: logged, left out
        PeakCluster([peak(1.0, 9.0, CAND_DM)], rank=3),
    ]
    cands = build_candidates_filterbank(clusters, fname, CAND_RANGES, DEREDDEN, nsub=CAND_NSUB)
    assert passes == [[CAND_DM, 0.0]]        # one pass, the distinct centre DMs by decreasing S/N
    assert [c.params["snr"] for c in cands] == [30.0, 12.0, 9.0]
    assert [c.params["dm"] for c in cands] == [CAND_DM, 0.0, CAND_DM]
    assert [c.tsmeta["dm"] for c in cands] == [CAND_DM, 0.0, CAND_DM]
    assert cands[0].tsmeta["fname"] == fb.metadata(0.0)["fname"] and cands[0].tsmeta["tobs"] == fb.tobs

    # the same folds, made here from band_series of the same arguments
    dms = [CAND_DM, 0.0]                                 # distinct centre DMs by decreasing S/N
    _, max_delay = dispersion_delays(fb.freqs, dms, fb.tsamp)
    nout = fb.nsamp - max_delay
    edges = band_edges(fb.nchans, CAND_NSUB)
    bands = np.concatenate([edges, np.array([[0, fb.nchans]], dtype=np.uint32)])
    series, _ = band_series(fb, dms, bands, DEREDDEN, nout)
    nb = len(bands)
    specs = [(i * nb + b, p, 64, 4) for i, p in ((0, CAND_PERIOD), (1, CAND_PERIOD), (0, 1.0)) for b in range(nb)]
    folds = [f.cpu().numpy() for f in engine.fold_device(series.view(2 * nb, nout), fb.tsamp, specs)]
    for k, c in enumerate(cands):
        assert c.subints.shape == (4, 64) and c.subints.dtype == np.float32
        assert c.subbands.shape == (CAND_NSUB, 4, 64) and c.subbands.dtype == np.float32
        assert np.array_equal(c.subints, folds[k * nb + nb - 1])
        assert np.array_equal(c.subbands, np.stack(folds[k * nb:k * nb + CAND_NSUB]))
        assert np.array_equal(c.band_freqs, [fb.freqs[lo:hi].mean() for lo, hi in edges])
        assert c.freq_phase.shape == (CAND_NSUB, 64)

    # dedispersed at its DM the pulse lines up across the band; at DM 0 it is
    # swept, later at lower frequencies (the bands go down in frequency)
    best = np.argmax(cands[0].freq_phase, axis=1)
    assert np.all(np.abs(best - np.argmax(cands[0].profile)) <= 1), best
    swept = np.argmax(cands[1].freq_phase, axis=1)
    assert np.all(np.diff(swept) > 0), swept

    # a budget whose half holds one DM's series (raw and normalised) and not
    # two, and which still has room for the gulp buffers of this small file:
    # two passes, the same candidates
    per_dm = 2 * nb * nout * 4
    two = build_candidates_filterbank(clusters, fb, CAND_RANGES, DEREDDEN, nsub=CAND_NSUB, budget_bytes=3 * per_dm)
    assert passes[1:] == [[CAND_DM], [0.0]] and len(two) == len(cands)
    for a, b in zip(cands, two):
        assert a.params == b.params and a.tsmeta["dm"] == b.tsmeta["dm"]
        assert np.array_equal(a.subints, b.subints) and np.array_equal(a.subbands, b.subbands)
    # nout: the search's own length
    cut = build_candidates_filterbank(clusters[:1], fb, CAND_RANGES, DEREDDEN, nsub=CAND_NSUB, nout=6000)
    assert len(cut) == 1 and cut[0].subbands.shape == (CAND_NSUB, 4, 64)
    assert not np.array_equal(cut[0].subints, cands[1].subints)
    assert build_candidates_filterbank([], fb, CAND_RANGES, DEREDDEN) == []
