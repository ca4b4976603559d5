"""GPU tests of the packed sample types (1, 2, 4 and 16 bit) on the filterbank
path: the unpack inside the transpose (csrc/dedisp_kernels.hip), the packed
readers of the zero-DM and statistics kernels, and the streamed and end-to-end
calls on a PackedFilterbank.  The reference is dedisp_common's numpy
restatement applied to reading.unpack_samples of the packed input, which
test_lowbit_host.py pins to the format's definition: bit for bit for 1/2/4
bit, within nchans * 2^-24 * sum |x| for 16 bit (float32 additions of exactly
converted values), which is bit for bit up to 256 channels."""
import numpy as np
import pytest

import dedisp_common as dc
from test_lowbit_host import write_packed

pytestmark = pytest.mark.gpu

DMS = [0.0, 50.0, 12.5, 50.0, 3.0]
# the host list (rows of 1, 3, 8 and 9 bytes) plus one channel count past a
# 64-byte tile of packed bytes (16 bit: past four 64-channel tiles)
CHANS = {1: (8, 24, 64, 72, 520), 2: (4, 12, 64, 68, 260), 4: (2, 6, 64, 66, 258), 16: (1, 3, 64, 65, 257)}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def packed(seed, nsamp, nchans, nbits):
    """(values [nsamp, nchans] as unpack_samples returns them, packed rows)."""
    from riptide_amd.reading import pack_samples, unpack_samples
    x = np.random.RandomState(seed).randint(0, 1 << nbits, size=(nsamp, nchans))
    x[nsamp // 2] = (1 << nbits) - 1
    raw = pack_samples(x, nbits)
    return unpack_samples(raw, nbits, nchans), raw


def run_block(torch, raw, nbits, delays, max_delay, mask=None, offset=0, **kw):
    """engine.dedisperse_device on packed rows placed `offset` bytes into a
    device allocation -> numpy."""
    from riptide_amd import engine
    buf = torch.zeros(raw.size + 8, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    block = buf[offset:offset + raw.size].view(raw.shape)
    block.copy_(torch.from_numpy(raw))
    assert block.data_ptr() % 4 == offset % 4
    d = torch.from_numpy(delays.astype(np.int32)).cuda()
    m = None if mask is None else torch.from_numpy(np.asarray(mask, dtype=np.uint8)).cuda()
    return engine.dedisperse_device(block, d, max_delay, mask=m, nbits=nbits, **kw).cpu().numpy()


def check(out, x, delays, nout, mask=None):
    """x: the unpacked values (uint8 or uint16)."""
    if x.dtype == np.uint16:
        xf = x.astype(np.float32)
        dc.assert_dedispersed(out, xf, delays, nout, mask)
        if x.shape[1] <= 256:      # integers below 2^24: every float32 addition is exact
            assert np.array_equal(out, dc.numpy_dedisperse(xf, delays, nout, mask)[0].astype(np.float32))
    else:
        dc.assert_dedispersed(out, x, delays, nout, mask)


@pytest.mark.parametrize("nbits,nchans", [(b, c) for b, chans in CHANS.items() for c in chans])
def test_channel_tiles(torch, nbits, nchans):
    """Rows narrower than a dword, not a multiple of 4 bytes (byte loads), a
    multiple (dword loads), and wider than the 64-byte tile; 600 outputs: two
    full time tiles and a partial one."""
    from riptide_amd.dedispersion import dispersion_delays
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS, dc.TSAMP)
    nout = 600
    x, raw = packed(nbits * 1000 + nchans, max_delay + nout, nchans, nbits)
    out = run_block(torch, raw, nbits, delays, max_delay)
    assert out.shape == (5, nout)
    check(out, x, delays, nout)


@pytest.mark.parametrize("nbits,nchans", [(1, 24), (2, 68)])
@pytest.mark.parametrize("nout", [1, 255, 256, 257, 1000])
def test_time_tiles(torch, nout, nbits, nchans):
    """Output counts around the 256-sample time tile, 3-byte rows (byte loads)
    and 17-byte rows; ascending band."""
    from riptide_amd.dedispersion import dispersion_delays
    delays, max_delay = dispersion_delays(dc.band(nchans, ascending=True), DMS, dc.TSAMP)
    x, raw = packed(nout, max_delay + nout, nchans, nbits)
    out = run_block(torch, raw, nbits, delays, max_delay)
    assert out.shape == (5, nout)
    check(out, x, delays, nout)


@pytest.mark.parametrize("nbits,nchans", [(1, 64), (2, 64), (4, 64), (16, 6), (4, 6)])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_alignment(torch, nbits, nchans, offset):
    """d_block is only byte-aligned: rows that are a multiple of 4 bytes take
    the byte loads when the block does not start on a dword."""
    from riptide_amd.dedispersion import dispersion_delays
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS, dc.TSAMP)
    nout = 300
    x, raw = packed(offset, max_delay + nout, nchans, nbits)
    out = run_block(torch, raw, nbits, delays, max_delay, offset=offset)
    check(out, x, delays, nout)
    assert np.array_equal(out, run_block(torch, raw, nbits, delays, max_delay))


@pytest.mark.parametrize("nbits,nchans", [(1, 72), (2, 68), (4, 66), (16, 65)])
def test_masks(torch, nbits, nchans):
    """First channel, last channel, and all but one."""
    from riptide_amd.dedispersion import dispersion_delays
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS, dc.TSAMP)
    nout = 300
    x, raw = packed(nbits, max_delay + nout, nchans, nbits)
    for sel in ([0], [nchans - 1], [c for c in range(nchans) if c != 5]):
        mask = np.zeros(nchans, dtype=bool)
        mask[sel] = True
        check(run_block(torch, raw, nbits, delays, max_delay, mask=mask), x, delays, nout, mask)


@pytest.mark.parametrize("nbits,nchans", [(1, 24), (2, 64), (4, 66), (16, 3)])
def test_no_over_read(torch, nbits, nchans):
    """The block is the first rows of a larger allocation whose remainder is
    0xFF: the result is that of the block alone.  (That no load passes the end
    of the allocation itself rests on the bounds argument of DESIGN.md 5a.2.)"""
    from riptide_amd import engine
    from riptide_amd.dedispersion import dispersion_delays
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS, dc.TSAMP)
    nout = 257
    nsamp = max_delay + nout
    x, raw = packed(nbits + nchans, nsamp, nchans, nbits)
    big = torch.full((nsamp + 300, raw.shape[1]), 255, dtype=torch.uint8, device="cuda")
    big[:nsamp] = torch.from_numpy(raw).cuda()
    d = torch.from_numpy(delays.astype(np.int32)).cuda()
    for zero_dm in (False, True):
        out = engine.dedisperse_device(big[:nsamp], d, max_delay, nbits=nbits, zero_dm=zero_dm).cpu().numpy()
        assert np.array_equal(out, run_block(torch, raw, nbits, delays, max_delay, zero_dm=zero_dm))
        if not zero_dm:
            check(out, x, delays, nout)
    zeros = torch.full((nsamp + 300, raw.shape[1]), 255, dtype=torch.uint8, device="cuda")
    zeros[:nsamp] = 0
    assert not engine.dedisperse_device(zeros[:nsamp], d, max_delay, nbits=nbits).cpu().numpy().any()


@pytest.mark.parametrize("nbits,nchans", [(1, 24), (1, 520), (2, 68), (4, 66), (16, 3), (16, 257)])
def test_zero_dm_and_statistics(torch, nbits, nchans):
    """1/2/4 bit: the mean series, the zero-DM sums and the statistics of the
    packed block equal those of the unpacked uint8 block, bit for bit.  16 bit:
    m is the float32 of the exact integer mean, the statistics are exact, and
    the zero-DM sums are within the float bound of the float64 sums of
    float32(x) - m.  2100 samples: two chunks of the statistics."""
    from riptide_amd import engine
    from riptide_amd.dedispersion import dispersion_delays
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS, dc.TSAMP)
    nsamp = 2100
    nout = nsamp - max_delay
    x, raw = packed(nbits * 7 + nchans, nsamp, nchans, nbits)
    block = torch.from_numpy(raw).cuda()
    d = torch.from_numpy(delays.astype(np.int32)).cuda()
    for mask in (None, np.arange(nchans) % 3 == 1 if nchans > 1 else None):
        keep = np.ones(nchans, dtype=bool) if mask is None else ~mask
        dm = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).cuda()
        m = engine.zero_dm_mean_device(block, mask=dm, nbits=nbits).cpu().numpy()
        out = engine.dedisperse_device(block, d, max_delay, mask=dm, zero_dm=True, nbits=nbits).cpu().numpy()
        m_ref = (x[:, keep].astype(np.int64).sum(axis=1).astype(np.float64) / keep.sum()).astype(np.float32)
        assert np.array_equal(m, m_ref)
        if nbits < 16:
            b8 = torch.from_numpy(x).cuda()
            assert np.array_equal(m, engine.zero_dm_mean_device(b8, mask=dm).cpu().numpy())
            assert np.array_equal(out, engine.dedisperse_device(b8, d, max_delay, mask=dm, zero_dm=True).cpu().numpy())
        else:
            y = x.astype(np.float32) - m[:, None]
            ref, mag = dc.numpy_dedisperse(y, delays, nout, mask)
            assert np.all(np.abs(out - ref) <= nchans * 2.0 ** -24 * mag)
    acc = torch.zeros((2, nchans), dtype=torch.float64, device="cuda")
    engine.channel_stats_device(block, acc, nbits=nbits)
    engine.channel_stats_device(block[:700], acc, nbits=nbits)      # accumulates
    xi = x.astype(np.int64)
    got = acc.cpu().numpy()
    assert np.array_equal(got[0], xi.sum(axis=0) + xi[:700].sum(axis=0))
    assert np.array_equal(got[1], (xi * xi).sum(axis=0) + (xi[:700] * xi[:700]).sum(axis=0))
    if nbits < 16:
        acc8 = torch.zeros((2, nchans), dtype=torch.float64, device="cuda")
        engine.channel_stats_device(torch.from_numpy(x).cuda(), acc8)
        engine.channel_stats_device(torch.from_numpy(x[:700]).cuda(), acc8)
        assert np.array_equal(got, acc8.cpu().numpy())


@pytest.mark.parametrize("nbits,nchans", [(1, 24), (2, 68), (4, 66), (16, 65)])
def test_gulp_independence(torch, tmp_path, nbits, nchans):
    """Gulps of max_delay + 1 samples, a prime, and the whole file give the
    same tensor, equal to dedisperse() of the packed host rows; the file-level
    mean series and statistics do not depend on the gulp either."""
    from riptide_amd import rfi
    from riptide_amd.dedispersion import dedisperse, dedisperse_filterbank, dispersion_delays
    from riptide_amd.reading import PackedFilterbank, open_filterbank
    nsamp = 1500
    x, raw = packed(nbits, nsamp, nchans, nbits)
    fb = open_filterbank(write_packed(tmp_path / "g.fil", x, nbits))
    assert isinstance(fb, PackedFilterbank)
    delays, max_delay = dispersion_delays(fb.freqs, DMS, dc.TSAMP)
    host = dedisperse(raw, fb.freqs, dc.TSAMP, DMS, nbits=nbits)
    check(host, x, delays, nsamp - max_delay)
    for zero_dm in (False, True):
        outs = [dedisperse_filterbank(fb, DMS, gulp=gulp, zero_dm=zero_dm).cpu().numpy()
                for gulp in (max_delay + 1, 1009, nsamp, None)]
        assert all(np.array_equal(o, outs[0]) for o in outs[1:])
        if not zero_dm:
            assert np.array_equal(outs[0], host)
    xi = x.astype(np.int64)
    for gulp in (7, 1009, None):
        st = rfi.channel_stats(fb, gulp=gulp)
        assert np.array_equal(st.sum, xi.sum(axis=0)) and np.array_equal(st.sumsq, (xi * xi).sum(axis=0))
        m = rfi.zero_dm_series(fb, gulp=gulp).cpu().numpy()
        assert np.array_equal(m, (xi.sum(axis=1).astype(np.float64) / nchans).astype(np.float32))


E2E_DMS = [0.0, 5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 35.0, 40.0]
E2E_DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}
E2E_RANGES = [{"name": "short",
               "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
               "find_peaks": {"smin": 7.0}}]


def test_search_filterbank_two_bit_equals_eight_bit(torch, tmp_path):
    """32 channels x 2^16 samples of 2-bit data, a train of 8-sample pulses of
    period 0.5 s swept at DM 20: search_filterbank of the file name gives the
    peak list of the same values written as an 8-bit file, with and without
    the zero-DM filter, and finds the pulsar."""
    import riptide_amd
    from riptide_amd.dispatch import EngineSearcher
    from riptide_amd.reading import write_sigproc
    nchans, nsamp = 32, 1 << 16
    rng = np.random.RandomState(4321)
    x = rng.normal(1.5, 0.8, size=(nsamp, nchans))
    sweep = dc.numpy_delays(dc.band(nchans), [20.0], dc.TSAMP)[0]
    for c in range(nchans):
        for t0 in range(100 + int(sweep[c]), nsamp - 8, 500):
            x[t0:t0 + 8, c] += 0.6
    x = np.clip(np.round(x), 0, 3).astype(np.uint8)
    f2 = write_packed(tmp_path / "two.fil", x, 2)
    f8 = str(tmp_path / "eight.fil")
    write_sigproc(f8, x, {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0,
                          "tsamp": dc.TSAMP, "nbits": 8, "fch1": 400.0, "foff": -1.0, "nchans": nchans, "nifs": 1})
    searcher = EngineSearcher(E2E_DEREDDEN, E2E_RANGES, device=0, batch=4)
    for zero_dm in (False, True):
        got = riptide_amd.search_filterbank(f2, E2E_DMS, searcher, zero_dm=zero_dm)
        ref = riptide_amd.search_filterbank(f8, E2E_DMS, searcher, zero_dm=zero_dm)
        assert len(got) > 0
        assert [tuple(p) for p in got] == [tuple(p) for p in ref]
        best = max(got, key=lambda p: p.snr)
        assert best.dm == 20.0 and abs(best.period - 0.5) <= 2 * 0.5 * (0.5 / 240) / (nsamp * dc.TSAMP), best


def test_errors(torch, tmp_path):
    """Every refusal is raised on the host, before any launch."""
    from riptide_amd import engine
    from riptide_amd.dedispersion import dedisperse, dedisperse_filterbank
    from riptide_amd.reading import open_filterbank
    block = torch.zeros((100, 3), dtype=torch.uint8, device="cuda")
    d24 = torch.zeros((1, 24), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="nbits 1, 2, 4 or 16"):
        engine.dedisperse_device(block, d24, 0, nbits=8)
    with pytest.raises(ValueError, match="whole number"):
        engine.dedisperse_device(block, d24, 0, nbits=16)
    with pytest.raises(ValueError, match="whole number"):
        engine.zero_dm_mean_device(block, nbits=16)
    with pytest.raises(ValueError, match="packed block must be uint8"):
        engine.dedisperse_device(block.to(torch.int8), d24, 0, nbits=1)
    with pytest.raises(ValueError, match="delays must be"):
        engine.dedisperse_device(block, d24, 0, nbits=2)             # 12 channels
    with pytest.raises(ValueError, match="max_delay"):
        engine.dedisperse_device(block, d24, 100, nbits=1)
    with pytest.raises(ValueError, match="workspace"):
        engine.dedisperse_device(block, d24, 0, nbits=1, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="acc must be"):
        engine.channel_stats_device(block, torch.zeros((2, 3), dtype=torch.float64, device="cuda"), nbits=1)
    wide = torch.zeros((2, 65800 // 2), dtype=torch.uint8, device="cuda")      # 65800 four-bit channels
    with pytest.raises(ValueError, match="2\\^24"):
        engine.dedisperse_device(wide, torch.zeros((1, 65800), dtype=torch.int32, device="cuda"), 0, nbits=4)
    with pytest.raises(ValueError, match="65793"):
        dedisperse(np.zeros((2, 65800 // 2), dtype=np.uint8), np.linspace(400.0, 368.0, 65800), dc.TSAMP, [0.0],
                   nbits=4)
    assert engine.dedisperse_workspace_bytes("u1", 1000, 24) == engine.dedisperse_workspace_bytes("uint8", 1000, 24)
    assert engine.dedisperse_workspace_bytes("u16", 1000, 24) == \
        engine.dedisperse_workspace_bytes("float32", 1000, 24, nbits=None)
    fb = open_filterbank(write_packed(tmp_path / "e.fil", np.zeros((1500, 8), dtype=np.uint8), 1))
    with pytest.raises(ValueError, match="largest delay"):
        dedisperse_filterbank(fb, [400.0])
    with pytest.raises(ValueError, match="gulp must exceed"):
        dedisperse_filterbank(fb, [50.0], gulp=10)
    with pytest.raises(ValueError, match="pass fewer DMs per call"):
        dedisperse_filterbank(fb, DMS, budget_bytes=20000)
