"""CPU-only tests of the RFI front end: the zero-DM specification
(rt_zero_dm_mean_host, rt_dedisperse_host_opt with RT_DEDISP_ZERO_DM) against
the numpy restatement of rfi_common, the channel statistics
(rt_channel_stats_host) against numpy sums, and rfi.channel_mask on a
synthetic band.  No call reaches the GPU."""
import ctypes

import numpy as np
import pytest

import dedisp_common as dc
import rfi_common as rc

DMS = (0.0, 50.0, 12.5, 50.0, 3.0)


@pytest.fixture(scope="module")
def lib():
    from riptide_amd import _lib
    return _lib.load()


def _masks(nchans):
    m = np.zeros(nchans, dtype=bool)
    m[[0, nchans // 2, nchans - 1]] = True
    return [None, m]


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.float32])
@pytest.mark.parametrize("nchans", [37, 65])
def test_zero_dm_specification(nchans, dtype):
    """m bit for bit for 8-bit data (an integer sum, one correctly rounded
    division); out within rfi_common.zero_dm_bound."""
    from riptide_amd.dedispersion import dedisperse_host, dispersion_delays, zero_dm_mean_host
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS, dc.TSAMP)
    nout = 257
    x = dc.samples(np.random.RandomState(nchans), max_delay + nout, nchans, dtype)
    for mask in _masks(nchans):
        m = zero_dm_mean_host(x, mask=mask)
        ref_m = rc.numpy_zero_dm_mean(x, mask)
        assert m.dtype == np.float32 and m.shape == (x.shape[0],)
        if dtype == np.float32:
            assert np.all(np.abs(m.astype(np.float64) - ref_m) <= 2.0 ** -23 * np.abs(ref_m))
        else:
            assert np.array_equal(m, ref_m)
        for n in (nout, 1):
            out = dedisperse_host(x, delays, max_delay, mask=mask, nout=n, zero_dm=True)
            rc.assert_zero_dm_dedispersed(out, x, delays, n, mask)
        # the plain call is what it was
        dc.assert_dedispersed(dedisperse_host(x, delays, max_delay, mask=mask), x, delays, nout, mask)


def test_zero_dm_properties():
    """DM 0 sums y over the channels its mean was taken over: zero up to the
    bound; one unmasked 8-bit channel is its own mean: exactly zero, at any
    DM.  No unmasked channel: m = 0 and out = 0."""
    from riptide_amd.dedispersion import dedisperse_host, dispersion_delays, zero_dm_mean_host
    nchans, nout = 37, 100
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS, dc.TSAMP)
    for dtype in (np.uint8, np.int8, np.float32):
        x = dc.samples(np.random.RandomState(3), max_delay + nout, nchans, dtype)
        out = dedisperse_host(x, delays, max_delay, zero_dm=True)
        ref, mag, magm = rc.numpy_zero_dm_dedisperse(x, rc.numpy_zero_dm_mean(x), delays, nout)
        assert np.all(np.abs(out[0]) <= rc.zero_dm_bound(x, delays, mag, magm)[0])
        one = np.ones(nchans, dtype=bool)
        one[20] = False
        if dtype != np.float32:
            assert np.array_equal(zero_dm_mean_host(x, mask=one), x[:, 20].astype(np.float32))
            assert not dedisperse_host(x, delays, max_delay, mask=one, zero_dm=True).any()
        every = np.ones(nchans, dtype=bool)
        assert not zero_dm_mean_host(x, mask=every).any()
        z = dedisperse_host(x, delays, max_delay, mask=every, zero_dm=True)
        assert z.shape == (len(DMS), nout) and not z.any()
        assert not dedisperse_host(x, delays, max_delay, mask=every).any()


def test_flags_zero_is_the_plain_call(lib):
    from riptide_amd import _lib
    from riptide_amd.dedispersion import dedisperse_host, dispersion_delays
    nchans, nout = 37, 64
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS, dc.TSAMP)
    for dtype, code in ((np.uint8, 0), (np.int8, 1), (np.float32, 2)):
        x = dc.samples(np.random.RandomState(1), max_delay + nout, nchans, dtype)
        old = np.zeros((len(DMS), nout), dtype=np.float32)
        assert lib.rt_dedisperse_host(_lib.ptr(x), code, x.shape[0], nchans, _lib.ptr(delays), None, len(DMS),
                                      max_delay, nout, _lib.ptr(old)) == _lib.RT_OK
        new = np.ones_like(old)
        assert lib.rt_dedisperse_host_opt(_lib.ptr(x), code, x.shape[0], nchans, _lib.ptr(delays), None, len(DMS),
                                          max_delay, nout, _lib.ptr(new), 0) == _lib.RT_OK
        assert np.array_equal(old, new) and np.array_equal(old, dedisperse_host(x, delays, max_delay))


@pytest.mark.parametrize("dtype,code", [(np.uint8, 0), (np.int8, 1), (np.float32, 2)])
def test_channel_stats_host(lib, dtype, code):
    """Two calls on the two halves add into one pair of accumulators.  8-bit:
    the int64 sums exactly.  float32: a float64 accumulation of n terms is
    within n * 2^-53 * sum |x| of the exact sum (squares: with sum x^2)."""
    from riptide_amd import _lib
    nsamp, nchans = 1001, 37
    x = dc.samples(np.random.RandomState(7), nsamp, nchans, dtype)
    acc = np.zeros((2, nchans), dtype=np.float64)
    half = 400
    for part in (x[:half], x[half:]):
        part = np.ascontiguousarray(part)
        assert lib.rt_channel_stats_host(_lib.ptr(part), code, part.shape[0], nchans, _lib.ptr(acc)) == _lib.RT_OK
    if dtype == np.float32:
        x64 = x.astype(np.float64)
        import math
        s = np.array([math.fsum(col) for col in x64.T])
        q = np.array([math.fsum(col * col) for col in x64.T])   # the squares of float32 values are exact in float64
        assert np.all(np.abs(acc[0] - s) <= nsamp * 2.0 ** -53 * np.abs(x64).sum(axis=0))
        assert np.all(np.abs(acc[1] - q) <= nsamp * 2.0 ** -53 * (x64 * x64).sum(axis=0))
    else:
        xi = x.astype(np.int64)
        assert np.array_equal(acc[0], xi.sum(axis=0).astype(np.float64))
        assert np.array_equal(acc[1], (xi * xi).sum(axis=0).astype(np.float64))


def _band_stats(std, mean, nsamp=1000):
    from riptide_amd.rfi import ChannelStats
    std, mean = np.asarray(std, dtype=np.float64), np.asarray(mean, dtype=np.float64)
    return ChannelStats(mean * nsamp, (std ** 2 + mean ** 2) * nsamp, nsamp)


def test_channel_mask():
    """64 channels with std 1 +- 0.02 and mean 100 +- 0.05 (uniform, so the
    MADs are about 0.01 and 0.025 and the 4 x 1.4826 x MAD cuts about 0.06 and
    0.15: beyond every good channel), plus a dead channel, one with 5 x the
    std and one with its mean shifted by 1: exactly those three."""
    from riptide_amd.rfi import channel_mask
    rng = np.random.RandomState(11)
    std = list(1.0 + rng.uniform(-0.02, 0.02, 64))
    mean = list(100.0 + rng.uniform(-0.05, 0.05, 64))
    bad = {5: (0.0, 0.0), 30: (5.0, 100.0), 50: (1.0, 101.0)}
    for at, (s, m) in sorted(bad.items()):
        std.insert(at, s)
        mean.insert(at, m)
    stats = _band_stats(std, mean)
    assert np.allclose(stats.std, std, atol=1e-9) and np.allclose(stats.mean, mean, atol=1e-9)
    mask = channel_mask(stats)
    assert mask.dtype == bool and mask.shape == (67,)
    assert sorted(np.flatnonzero(mask)) == sorted(bad)
    assert sorted(np.flatnonzero(channel_mask(stats, threshold=4.0, max_iter=1))) == sorted(bad)
    # an all-equal band: MAD 0, nothing flagged
    assert not channel_mask(_band_stats(np.full(64, 2.0), np.full(64, 7.0))).any()
    # every channel dead: all flagged, no median of nothing
    assert channel_mask(_band_stats(np.zeros(8), np.zeros(8))).all()


def test_errors(lib):
    from riptide_amd import _lib
    from riptide_amd.dedispersion import dedisperse_host, zero_dm_mean_host
    x = np.ones((10, 2), dtype=np.uint8)
    d = np.array([[0, 3]], dtype=np.int64)
    out = np.zeros((1, 7), dtype=np.float32)
    # an unknown flag bit
    assert lib.rt_dedisperse_host_opt(_lib.ptr(x), 0, 10, 2, _lib.ptr(d), None, 1, 3, 7, _lib.ptr(out),
                                      2) == _lib.RT_EINVAL
    assert b"unknown flag bit" in lib.rt_last_error()
    assert lib.rt_dedisperse_host_opt(_lib.ptr(x), 0, 10, 2, _lib.ptr(d), None, 1, 3, 7, _lib.ptr(out),
                                      3) == _lib.RT_EINVAL
    b = ctypes.c_size_t()
    assert lib.rt_dedisperse_workspace_bytes_opt(0, 1001, 37, 4, ctypes.byref(b)) == _lib.RT_EINVAL
    # the flagged workspace: float rows for every dtype, plus nsamp_blk floats (16-byte aligned) for m
    for code in (0, 1, 2):
        assert lib.rt_dedisperse_workspace_bytes_opt(code, 1001, 37, 1, ctypes.byref(b)) == _lib.RT_OK
        assert b.value == 4016 * 37 + 4016
    assert lib.rt_dedisperse_workspace_bytes_opt(0, 1001, 37, 0, ctypes.byref(b)) == _lib.RT_OK and b.value == 1008 * 37
    # the flag with more than 65793 8-bit channels
    wide = np.zeros((1, 65794), dtype=np.uint8)
    dw = np.zeros((1, 65794), dtype=np.int64)
    ow = np.zeros((1, 1), dtype=np.float32)
    assert lib.rt_dedisperse_host_opt(_lib.ptr(wide), 0, 1, 65794, _lib.ptr(dw), None, 1, 0, 1, _lib.ptr(ow),
                                      1) == _lib.RT_EINVAL
    assert b"too many channels" in lib.rt_last_error()
    assert lib.rt_dedisperse_workspace_bytes_opt(1, 1001, 65794, 1, ctypes.byref(b)) == _lib.RT_EINVAL
    mw = np.zeros(1, dtype=np.float32)
    assert lib.rt_zero_dm_mean_host(_lib.ptr(wide), 0, 1, 65794, None, _lib.ptr(mw)) == _lib.RT_EINVAL
    with pytest.raises(ValueError, match="65793"):
        dedisperse_host(wide, dw, 0, zero_dm=True)
    wide32 = wide.astype(np.float32)
    assert lib.rt_dedisperse_host_opt(_lib.ptr(wide32), 2, 1, 65794, _lib.ptr(dw), None, 1, 0, 1, _lib.ptr(ow),
                                      1) == _lib.RT_OK
    # the mask's length
    with pytest.raises(ValueError, match="one entry per channel"):
        dedisperse_host(x, d, 3, mask=[True], zero_dm=True)
    with pytest.raises(ValueError, match="one entry per channel"):
        zero_dm_mean_host(x, mask=[True, False, True])
    # the statistics
    acc = np.zeros((2, 2), dtype=np.float64)
    assert lib.rt_channel_stats_host(_lib.ptr(x), 9, 10, 2, _lib.ptr(acc)) == _lib.RT_EINVAL
    assert lib.rt_channel_stats_host(_lib.ptr(x), 0, 10, 0, _lib.ptr(acc)) == _lib.RT_EINVAL
    assert lib.rt_channel_stats_host(_lib.ptr(x), 0, 10, 2, None) == _lib.RT_EINVAL
    assert not acc.any()
