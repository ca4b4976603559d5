"""CPU-only tests of the sub-band dedispersion specification
(rt_dedisperse_bands_host) against the numpy restatement of dedisp_common with
a per-band mask, its argument errors, band_edges, the Candidate fields that
carry the band folds, and the sanitizer program.  No call reaches the GPU."""
import os
import subprocess

import numpy as np
import pytest

import dedisp_common as dc
from conftest import REPO

NCHANS = 37
DMS = (0.0, 50.0, 12.5, 50.0, 3.0)
# around the kernel's 16-channel step: overlapping, one empty, unsorted
BANDS = np.array([[0, 1], [0, 16], [5, 21], [15, 17], [16, 32], [20, 37], [36, 37], [0, 37], [9, 9]], dtype=np.uint32)


def band_mask(lo, hi, mask, nchans):
    """The channel mask that leaves band [lo, hi) of what `mask` leaves."""
    m = np.ones(nchans, dtype=bool)
    m[lo:hi] = False
    return m if mask is None else m | np.asarray(mask, dtype=bool)


def zero_dm_rows(x, mask):
    """y = float32(x) - m as include/riptide_amd.h defines it, m from
    rt_zero_dm_mean_host (pinned by test_rfi_host.py)."""
    from riptide_amd.dedispersion import zero_dm_mean_host
    return x.astype(np.float32) - zero_dm_mean_host(x, mask=mask)[:, None]


def assert_band_rows(out, x, delays, nout, bands, mask=None):
    """out [ndm, nbands, nout] against dc.numpy_dedisperse with each band's
    mask: bit for bit for integer data, within (band width) * 2^-24 * sum |x|
    (dc.assert_dedispersed's bound with the band's width for nchans) for float."""
    assert out.dtype == np.float32 and out.shape == (delays.shape[0], len(bands), nout)
    for b, (lo, hi) in enumerate(bands):
        ref, mag = dc.numpy_dedisperse(x, delays, nout, band_mask(lo, hi, mask, x.shape[1]))
        if x.dtype == np.float32:
            err = np.abs(out[:, b].astype(np.float64) - ref)
            bound = (int(hi) - int(lo)) * 2.0 ** -24 * mag
            assert np.all(np.isfinite(out[:, b])) and np.all(err <= bound), \
                f"band {b}: max excess {float((err - bound).max()):.3e}"
        else:
            assert np.array_equal(out[:, b], ref.astype(np.float32)), f"band {b} differs"


def make_input(kind, nsamp, seed=0):
    """(what the entry point takes, its values [nsamp, NCHANS], nbits) of a sample type."""
    rng = np.random.RandomState(seed)
    if kind == "u2":
        from riptide_amd.reading import pack_samples
        nchans = 36                       # whole bytes of 2-bit samples
        vals = rng.randint(0, 4, size=(nsamp, nchans)).astype(np.uint8)
        return pack_samples(vals, 2), vals, 2
    x = dc.samples(rng, nsamp, NCHANS, kind)
    return x, x, None


@pytest.mark.parametrize("zero_dm", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", ["uint8", "int8", "float32", "u2"])
def test_host_specification(kind, masked, zero_dm):
    from riptide_amd.dedispersion import dedisperse_bands_host, dedisperse_host, dispersion_delays
    nout = 60
    nchans = 36 if kind == "u2" else NCHANS
    bands = np.minimum(BANDS, nchans)
    delays, max_delay = dispersion_delays(dc.band(nchans), DMS, dc.TSAMP)
    data, vals, nbits = make_input(kind, max_delay + nout, seed=masked + 2 * zero_dm)
    mask = None
    if masked:
        mask = np.zeros(nchans, dtype=bool)
        mask[[0, 15, 16, 35]] = True
    out = dedisperse_bands_host(data, delays, max_delay, bands, mask=mask, nout=nout, zero_dm=zero_dm, nbits=nbits)
    if zero_dm:
        # the filtered rows are float32 data of the plain sum: the mean is over
        # the unmasked channels of the whole file, not of the band
        assert_band_rows(out, zero_dm_rows(vals, mask), delays, nout, bands, mask)
    else:
        assert_band_rows(out, vals, delays, nout, bands, mask)
    # the full band is the plain specification, bit for bit; an empty band is zero
    plain = dedisperse_host(data, delays, max_delay, mask=mask, nout=nout, zero_dm=zero_dm, nbits=nbits)
    assert np.array_equal(out[:, 7], plain)
    assert not out[:, 8].any()


def test_argument_errors():
    from riptide_amd import _lib
    from riptide_amd.dedispersion import dedisperse_bands_host
    lib = _lib.load()
    nchans, nout = 8, 10
    x = np.ones((20, nchans), dtype=np.uint8)
    delays = np.full((2, nchans), 3, dtype=np.int64)
    ok = [[0, 4], [4, 8]]
    assert np.all(dedisperse_bands_host(x, delays, 3, ok, nout=nout) == 4.0)
    assert dedisperse_bands_host(x, delays, 3, np.zeros((0, 2), dtype=np.uint32), nout=nout).shape == (2, 0, nout)
    cases = [
        (dict(bands=[[0, 4], [5, 4]]), r"band 1 \[5, 4\) is not a channel range lo <= hi <= 8"),
        (dict(bands=[[0, 4], [4, 9]]), r"band 1 \[4, 9\) is not a channel range lo <= hi <= 8"),
        (dict(nout=18), "nout \\+ max_delay exceeds the 20 samples"),
        (dict(max_delay=2), "a delay is outside"),
        (dict(max_delay=-1), "max_delay is outside"),
        (dict(data=x[:, :0]), "nchans and ndm must be at least 1"),
        (dict(delays=delays[:0]), "nchans and ndm must be at least 1"),
    ]
    for change, text in cases:
        kw = dict(data=x, delays=delays, max_delay=3, bands=ok, nout=nout)
        kw.update(change)
        if kw["data"].shape[1] == 0:
            kw["delays"] = np.zeros((2, 0), dtype=np.int64)
        with pytest.raises(ValueError, match=text):
            dedisperse_bands_host(**kw)
    # what the Python layer cannot express: an unknown type code, a flag bit,
    # a NULL table, packed rows that are not whole bytes
    out = np.zeros((2, 2, nout), dtype=np.float32)
    b = np.asarray(ok, dtype=np.uint32)

    def call(dtype, bands, flags, nch=nchans):
        return lib.rt_dedisperse_bands_host(_lib.ptr(x), dtype, 20, nch, _lib.ptr(delays), None, 2, bands, 2, 3, nout,
                                            _lib.ptr(out), flags)
    assert call(0, _lib.ptr(b), 0) == _lib.RT_OK
    assert call(7, _lib.ptr(b), 0) == _lib.RT_EINVAL and b"unknown sample type code" in lib.rt_last_error()
    assert call(0, _lib.ptr(b), 2) == _lib.RT_EINVAL and b"unknown flag bit" in lib.rt_last_error()
    assert call(0, None, 0) == _lib.RT_EINVAL and b"bands is NULL" in lib.rt_last_error()
    b3 = np.array([[0, 1], [1, 3]], dtype=np.uint32)
    assert call(0x102, _lib.ptr(b3), 0, nch=3) == _lib.RT_EINVAL and b"not a whole number of bytes" in lib.rt_last_error()


def test_band_edges():
    from riptide_amd.dedispersion import band_edges
    for nsub in (1, 5, 37):
        e = band_edges(37, nsub)
        assert e.dtype == np.uint32 and e.shape == (nsub, 2)
        assert [tuple(r) for r in e] == [(s * 37 // nsub, (s + 1) * 37 // nsub) for s in range(nsub)]
        assert e[0, 0] == 0 and e[-1, 1] == 37 and np.array_equal(e[1:, 0], e[:-1, 1])    # a partition
        assert np.all(e[:, 1] > e[:, 0])
    assert [tuple(r) for r in band_edges(37, 5)] == [(0, 7), (7, 14), (14, 22), (22, 29), (29, 37)]
    for nsub in (0, 38, -1):
        with pytest.raises(ValueError, match="nsub must be in"):
            band_edges(37, nsub)


def test_candidate_round_trip_with_subbands():
    from riptide_amd import Candidate
    rng = np.random.RandomState(5)
    sub = rng.normal(size=(4, 16)).astype(np.float32)
    bands = rng.normal(size=(3, 4, 16)).astype(np.float32)
    freqs = np.array([395.0, 385.0, 372.0])
    plain = Candidate({"snr": 9.0}, {"dm": 5.0}, "peaks", sub)
    assert plain.subbands is None and plain.band_freqs is None and plain.freq_phase is None
    d = plain.to_dict()
    assert set(d) == {"params", "tsmeta", "peaks", "subints"}
    back = Candidate.from_dict(d)
    assert back.subints is sub and back.subbands is None and back.band_freqs is None
    c = Candidate({"snr": 9.0}, {"dm": 5.0}, "peaks", sub, subbands=bands, band_freqs=freqs)
    d = c.to_dict()
    assert set(d) == {"params", "tsmeta", "peaks", "subints", "subbands", "band_freqs"}
    back = Candidate.from_dict(d)
    assert back.subints is sub and back.subbands is bands and back.band_freqs is freqs
    assert c.freq_phase.shape == (3, 16) and np.array_equal(c.freq_phase, bands.sum(axis=1))
    flat = Candidate({"snr": 1.0}, {}, None, sub[0], subbands=bands[:, 0], band_freqs=freqs)
    assert flat.freq_phase is flat.subbands


def test_asan_bands_check():
    """`make asan` builds build/asan/bands_check (g++, AddressSanitizer +
    UBSan, no HIP): rt_dedisperse_bands_host on exact-size heap arrays with
    an empty band, one-channel bands, the full band and bands ending at
    nchans, and every error return."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "bands_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("bands_check OK")
