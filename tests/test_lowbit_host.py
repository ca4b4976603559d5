"""CPU-only tests of the packed sample types (1, 2, 4 and 16 bit): the numpy
pack / unpack pair against a per-sample loop written from the format's
definition, the PackedFilterbank reader, the error returns, and the host
specification on packed rows against the same calls on the unpacked values.
No call reaches the GPU."""
import ctypes

import numpy as np
import pytest

import dedisp_common as dc

# nbits -> channel counts whose rows are 1, 3 and 9 (16 bit: 2, 6, 130) bytes
SHAPES = {1: (8, 24, 72), 2: (4, 12, 68), 4: (2, 6, 66), 16: (1, 3, 65)}
CASES = [(nbits, nchans) for nbits, chans in SHAPES.items() for nchans in chans]
CODES = {1: 0x101, 2: 0x102, 4: 0x104, 16: 0x110}


@pytest.fixture(scope="module")
def lib():
    from riptide_amd import _lib
    return _lib.load()


def loop_unpack(raw, nbits, nchans):
    """The definition, sample by sample."""
    out = np.zeros((raw.shape[0], nchans), dtype=np.int64)
    for t in range(raw.shape[0]):
        row = [int(b) for b in raw[t]]
        for c in range(nchans):
            if nbits == 16:
                out[t, c] = row[2 * c] | row[2 * c + 1] << 8
            else:
                out[t, c] = (row[(c * nbits) >> 3] >> ((c * nbits) & 7)) & ((1 << nbits) - 1)
    return out


def patterns(nbits, nchans, nrows=5):
    t, c = np.meshgrid(np.arange(nrows), np.arange(nchans), indexing="ij")
    yield np.full((nrows, nchans), (1 << nbits) - 1, dtype=np.int64)
    yield (7 * c + 3 * t) % (1 << nbits)
    yield np.random.RandomState(nbits * 1000 + nchans).randint(0, 1 << nbits, size=(nrows, nchans))


@pytest.mark.parametrize("nbits,nchans", CASES)
def test_pack_unpack(nbits, nchans):
    from riptide_amd.reading import pack_samples, unpack_samples
    for x in patterns(nbits, nchans):
        raw = pack_samples(x, nbits)
        assert raw.dtype == np.uint8 and raw.shape == (5, nchans * nbits // 8)
        assert np.array_equal(loop_unpack(raw, nbits, nchans), x)
        back = unpack_samples(raw, nbits, nchans)
        assert back.dtype == (np.uint16 if nbits == 16 else np.uint8) and back.shape == x.shape
        assert back.flags.c_contiguous
        assert np.array_equal(back, x)
        assert np.array_equal(unpack_samples(raw.ravel(), nbits, nchans), x)     # flat bytes
    # arbitrary bytes unpack as the definition says (and pack back to themselves)
    raw = np.random.RandomState(nchans).randint(0, 256, size=(5, nchans * nbits // 8)).astype(np.uint8)
    vals = unpack_samples(raw, nbits, nchans)
    assert np.array_equal(vals, loop_unpack(raw, nbits, nchans))
    assert np.array_equal(pack_samples(vals, nbits), raw)


def test_pack_errors():
    from riptide_amd.reading import pack_samples, unpack_samples
    with pytest.raises(ValueError, match="whole number of bytes"):
        pack_samples(np.zeros((3, 12), dtype=np.uint8), 1)
    with pytest.raises(ValueError, match="whole number of bytes"):
        pack_samples(np.zeros((3, 3), dtype=np.uint8), 4)
    with pytest.raises(ValueError, match="whole number of bytes"):
        unpack_samples(np.zeros(6, dtype=np.uint8), 2, 6)
    with pytest.raises(ValueError, match="must be in"):
        pack_samples(np.full((2, 4), 4, dtype=np.uint8), 2)
    with pytest.raises(ValueError, match="must be in"):
        pack_samples(np.full((2, 4), -1, dtype=np.int64), 4)
    with pytest.raises(ValueError, match="must be in"):
        pack_samples(np.full((2, 4), 65536, dtype=np.int64), 16)
    with pytest.raises(ValueError, match="nbits"):
        pack_samples(np.zeros((2, 8), dtype=np.uint8), 8)
    with pytest.raises(ValueError, match="integer"):
        pack_samples(np.zeros((2, 8), dtype=np.float32), 1)


def write_packed(path, x, nbits, foff=-1.0, **extra):
    """x [nsamp, nchans] values -> a SIGPROC file of packed rows, written as
    1-D bytes."""
    from riptide_amd.reading import pack_samples, write_sigproc
    nchans = x.shape[1]
    step = 32.0 / nchans
    header = {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": dc.TSAMP,
              "nbits": nbits, "fch1": 400.0 if foff < 0 else 368.0, "foff": -step if foff < 0 else step,
              "nchans": nchans, "nifs": 1}
    header.update(extra)
    write_sigproc(str(path), pack_samples(x, nbits).ravel(), header)
    return str(path)


@pytest.mark.parametrize("foff", [-1.0, 1.0])
@pytest.mark.parametrize("nbits", [1, 2, 4, 16])
def test_open_filterbank(tmp_path, nbits, foff):
    import riptide_amd
    from riptide_amd.reading import Filterbank, PackedFilterbank, open_filterbank
    assert riptide_amd.open_filterbank is open_filterbank and riptide_amd.PackedFilterbank is PackedFilterbank
    nchans, nsamp = SHAPES[nbits][2], 41
    x = np.random.RandomState(nbits).randint(0, 1 << nbits, size=(nsamp, nchans))
    extra = {"signed": True} if nbits == 2 else {}       # ignored on 1/2/4 bit
    fb = open_filterbank(write_packed(tmp_path / "p.fil", x, nbits, foff, **extra))
    assert isinstance(fb, PackedFilterbank) and isinstance(fb, Filterbank)
    assert (fb.nsamp, fb.nchans, fb.nbits, fb.row_bytes) == (nsamp, nchans, nbits, nchans * nbits // 8)
    assert fb.dtype == (np.uint16 if nbits == 16 else np.uint8)
    assert np.array_equal(fb.freqs, dc.band(nchans, ascending=foff > 0))
    assert fb.tsamp == dc.TSAMP and fb.tobs == nsamp * dc.TSAMP
    assert fb.metadata(dm=3.0)["dm"] == 3.0 and fb.metadata()["tobs"] == fb.tobs
    assert isinstance(fb.data, np.memmap) and fb.data.dtype == np.uint8 and fb.data.shape == (nsamp, fb.row_bytes)
    assert not fb.data.flags.writeable
    with pytest.raises(ValueError):
        fb.data[0, 0] = 1
    assert np.array_equal(fb.unpack(), x) and fb.unpack().dtype == fb.dtype
    assert np.array_equal(fb.unpack(7, 19), x[7:19])
    assert np.array_equal(fb.unpack(30), x[30:])


def test_open_filterbank_plain_widths(tmp_path):
    from riptide_amd.reading import Filterbank, PackedFilterbank, open_filterbank, write_sigproc
    x = np.arange(60, dtype=np.uint8).reshape(10, 6)
    header = {"tsamp": dc.TSAMP, "nbits": 8, "fch1": 400.0, "foff": -1.0, "nchans": 6, "nifs": 1}
    fname = str(tmp_path / "u8.fil")
    write_sigproc(fname, x, header)
    fb = open_filterbank(fname)
    assert type(fb) is Filterbank and np.array_equal(fb.data, x)
    write_sigproc(fname, x.astype(np.float32), dict(header, nbits=32))
    fb = open_filterbank(fname)
    assert type(fb) is Filterbank and fb.dtype == np.float32
    with pytest.raises(ValueError, match="not 1-, 2-, 4- or 16-bit"):
        PackedFilterbank(fname)


def test_reader_errors(tmp_path):
    from riptide_amd.reading import Filterbank, PackedFilterbank, open_filterbank, write_sigproc
    header = {"tsamp": dc.TSAMP, "fch1": 400.0, "foff": -1.0, "nifs": 1}
    fname = str(tmp_path / "bad.fil")
    raw = np.zeros(30, dtype=np.uint8)
    for nbits, nchans in ((1, 12), (2, 6), (4, 3)):
        write_sigproc(fname, raw, dict(header, nbits=nbits, nchans=nchans))
        with pytest.raises(ValueError, match="rows are not a whole number of bytes"):
            open_filterbank(fname)
    write_sigproc(fname, raw, dict(header, nbits=16, nchans=3, signed=True))
    with pytest.raises(ValueError, match="signed 16-bit"):
        open_filterbank(fname)
    write_sigproc(fname, raw, dict(header, nbits=16, nchans=3, signed=False))
    assert open_filterbank(fname).nsamp == 5
    write_sigproc(fname, raw, dict(header, nbits=2, nchans=4, nifs=2))
    with pytest.raises(ValueError, match="nifs = 2"):
        open_filterbank(fname)
    with pytest.raises(ValueError, match="nifs = 2"):
        PackedFilterbank(fname)
    # the plain class still refuses packed data, in its own words
    write_sigproc(fname, raw, dict(header, nbits=2, nchans=4))
    with pytest.raises(ValueError, match="contains 2-bit data"):
        Filterbank(fname)
    write_sigproc(fname, raw, dict(header, nbits=3, nchans=8))
    with pytest.raises(ValueError, match="contains 3-bit data"):
        open_filterbank(fname)


def test_row_bytes(lib):
    from riptide_amd import _lib

    def row_bytes(code, nchans):
        b = ctypes.c_size_t(12345)
        return lib.rt_dedisp_row_bytes(code, nchans, ctypes.byref(b)), b.value

    assert row_bytes(0, 7) == (_lib.RT_OK, 7)
    assert row_bytes(1, 7) == (_lib.RT_OK, 7)
    assert row_bytes(2, 7) == (_lib.RT_OK, 28)
    for nbits, chans in SHAPES.items():
        for nchans in chans:
            assert row_bytes(CODES[nbits], nchans) == (_lib.RT_OK, nchans * nbits // 8)
    for code, nchans in ((0x101, 12), (0x102, 6), (0x104, 3), (0x101, 1)):
        assert row_bytes(code, nchans)[0] == _lib.RT_EINVAL
        assert b"rows are not a whole number of bytes" in lib.rt_last_error()
    for code in (5, 7, 9, 0x100, 0x103, 0x108, 0x120):
        assert row_bytes(code, 8)[0] == _lib.RT_EINVAL
    assert row_bytes(0x104, 0)[0] == _lib.RT_EINVAL
    assert lib.rt_dedisp_row_bytes(0x104, 2, None) == _lib.RT_EINVAL


def test_c_abi_errors(lib):
    """The new codes with a bad nchans, through every entry point that takes a
    type code without a device (the workspace queries only check the shape)."""
    from riptide_amd import _lib
    x = np.zeros(64, dtype=np.uint8)
    out = np.zeros(16, dtype=np.float32)
    acc = np.zeros(32, dtype=np.float64)
    delays = np.zeros(16, dtype=np.int64)
    b = ctypes.c_size_t()
    for code, nchans in ((0x101, 12), (0x102, 6), (0x104, 3)):
        calls = [
            lambda: lib.rt_dedisperse_host(_lib.ptr(x), code, 4, nchans, _lib.ptr(delays), None, 1, 0, 4, _lib.ptr(out)),
            lambda: lib.rt_dedisperse_host_opt(_lib.ptr(x), code, 4, nchans, _lib.ptr(delays), None, 1, 0, 4,
                                               _lib.ptr(out), 1),
            lambda: lib.rt_zero_dm_mean_host(_lib.ptr(x), code, 4, nchans, None, _lib.ptr(out)),
            lambda: lib.rt_channel_stats_host(_lib.ptr(x), code, 4, nchans, _lib.ptr(acc)),
            lambda: lib.rt_dedisperse_workspace_bytes(code, 100, nchans, ctypes.byref(b)),
            lambda: lib.rt_dedisperse_workspace_bytes_opt(code, 100, nchans, 1, ctypes.byref(b)),
        ]
        for call in calls:
            assert call() == _lib.RT_EINVAL
            assert b"rows are not a whole number of bytes" in lib.rt_last_error()
    # the 8-bit channel cap holds for 1/2/4 bit and not for 16 bit
    assert lib.rt_dedisperse_workspace_bytes(0x104, 100, 65794, ctypes.byref(b)) == _lib.RT_EINVAL
    assert b"2^24" in lib.rt_last_error()
    assert lib.rt_dedisperse_workspace_bytes(0x104, 100, 65792, ctypes.byref(b)) == _lib.RT_OK
    assert lib.rt_dedisperse_workspace_bytes(0x110, 100, 65794, ctypes.byref(b)) == _lib.RT_OK
    # workspace sizes: the 8-bit size for 1/2/4 bit, the float size for 16 bit, the zero-DM size with the flag
    sizes = {}
    for code in (0, 2, 0x101, 0x102, 0x104, 0x110):
        for flags in (0, 1):
            assert lib.rt_dedisperse_workspace_bytes_opt(code, 1000, 24, flags, ctypes.byref(b)) == _lib.RT_OK
            sizes[code, flags] = b.value
    assert sizes[0x101, 0] == sizes[0x102, 0] == sizes[0x104, 0] == sizes[0, 0] == 1008 * 24
    assert sizes[0x110, 0] == sizes[2, 0] == 4000 * 24
    assert len({sizes[code, 1] for code in (0, 2, 0x101, 0x102, 0x104, 0x110)}) == 1
    # Python level
    from riptide_amd.dedispersion import dedisperse_host, zero_dm_mean_host
    with pytest.raises(ValueError, match="nbits must be"):
        dedisperse_host(np.zeros((4, 3), dtype=np.uint8), np.zeros((1, 3), dtype=np.int64), 0, nbits=8)
    with pytest.raises(ValueError, match="whole number"):
        zero_dm_mean_host(np.zeros((4, 3), dtype=np.uint8), nbits=16)
    with pytest.raises(ValueError, match="uint8"):
        zero_dm_mean_host(np.zeros((4, 4), dtype=np.int8), nbits=4)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nbits", [1, 2, 4, 16])
def test_host_specification_on_packed_rows(lib, nbits, masked):
    """37 rows x 24 channels, 3 DMs.  1/2/4 bit: every call on the packed rows
    equals the same call on the unpacked values as uint8, bit for bit.  16
    bit: the plain sum equals the call on the values as float32 (the same
    float32 additions), the mean and the statistics are checked against exact
    integer arithmetic."""
    from riptide_amd import _lib
    from riptide_amd.dedispersion import dedisperse_host, dispersion_delays, zero_dm_mean_host
    from riptide_amd.reading import pack_samples
    nsamp, nchans = 37, 24
    x = np.random.RandomState(nbits + 10 * masked).randint(0, 1 << nbits, size=(nsamp, nchans))
    x[3] = (1 << nbits) - 1
    raw = pack_samples(x, nbits)
    delays, max_delay = dispersion_delays(dc.band(nchans), [0.0, 2.5, 1.0], dc.TSAMP)
    assert 0 < max_delay < nsamp - 5
    mask = None
    if masked:
        mask = np.zeros(nchans, dtype=bool)
        mask[[0, 7, nchans - 1]] = True
    keep = np.ones(nchans, dtype=bool) if mask is None else ~mask

    def stats(data, code):
        acc = np.zeros((2, nchans), dtype=np.float64)
        assert lib.rt_channel_stats_host(_lib.ptr(data), code, nsamp, nchans, _lib.ptr(acc)) == _lib.RT_OK
        return acc

    got = dedisperse_host(raw, delays, max_delay, mask=mask, nbits=nbits)
    got_zdm = dedisperse_host(raw, delays, max_delay, mask=mask, zero_dm=True, nbits=nbits)
    got_m = zero_dm_mean_host(raw, mask=mask, nbits=nbits)
    got_stats = stats(raw, CODES[nbits])
    assert got.shape == got_zdm.shape == (3, nsamp - max_delay)
    if nbits < 16:
        x8 = x.astype(np.uint8)
        assert np.array_equal(got, dedisperse_host(x8, delays, max_delay, mask=mask))
        assert np.array_equal(got_zdm, dedisperse_host(x8, delays, max_delay, mask=mask, zero_dm=True))
        assert np.array_equal(got_m, zero_dm_mean_host(x8, mask=mask))
        assert np.array_equal(got_stats, stats(x8, 0))
        dc.assert_dedispersed(got, x8, delays, nsamp - max_delay, mask)
    else:
        assert np.array_equal(got, dedisperse_host(x.astype(np.float32), delays, max_delay, mask=mask))
        m = (x[:, keep].sum(axis=1).astype(np.float64) / keep.sum()).astype(np.float32)
        assert np.array_equal(got_m, m)
        assert np.array_equal(got_stats[0], x.sum(axis=0)) and np.array_equal(got_stats[1], (x * x).sum(axis=0))
        # y = float32(x) - m, summed in float32 in channel order: the float path on x - m
        y = x.astype(np.float32) - m[:, None]
        ref, mag = dc.numpy_dedisperse(y, delays, nsamp - max_delay, mask)
        assert np.all(np.abs(got_zdm - ref) <= nchans * 2.0 ** -24 * mag)
