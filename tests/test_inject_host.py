"""Signal injection without a device: rt_inject_host against the numpy
restatement of inject_common at every shape, kind, factor and edge, saturation,
gulp independence, the dither's statistics, the amplitude normalisation and
exact recovery through dedisperse_host, every refusal with nothing written, the
Python layer's argument checks, and the sanitizer build of the checker."""
import os
import subprocess

import numpy as np
import pytest

import dedisp_common as dc
import inject_common as ic
from conftest import REPO


def _raw_host(x, specs, tmpl, amp, delay, t_origin=0, seed=0, code=0):
    """rt_inject_host on raw arrays, in place: the return code."""
    from riptide_amd import _lib
    L = _lib.load()
    return L.rt_inject_host(_lib.ptr(x), code, x.shape[0], x.shape[1], t_origin, seed, _lib.ptr(specs), specs.size,
                            _lib.ptr(tmpl), tmpl.size, _lib.ptr(amp), amp.size, _lib.ptr(delay), delay.size)


CASES = ((0, 1), (1, 1), (3, 10), (3, 16), (1, 16), (3, 1), (9, 10))      # (K, log2bins)


@pytest.mark.parametrize("nchans", ic.NCHANS)
@pytest.mark.parametrize("dtype", ic.DTYPES)
def test_host_equals_numpy(dtype, nchans):
    """Bit for bit over g, t_origin, K (both kinds mixed) and log2bins.  The
    K = 9 case has every factor (0, +-edge, +-small) and a pulse window partly
    before row 0, partly past the last row, wholly outside and inside
    (asserted on the very tables at g = 63 and 257; one row cannot be
    straddled), a phase that wraps inside the block, and from 63 channels on
    delays below zero and above the block's length."""
    from riptide_amd.injection import InjectionTables, inject_host
    for g in (1, 63, 257):
        x = ic.block(g, nchans, dtype)
        for t_origin in (0, 1000):
            for K, log2bins in CASES:
                raw = ic.raw_tables(K, nchans, g, t_origin, log2bins)
                if K == 9 and g > 1:
                    ic.covers_edges(raw, g, t_origin)
                    if nchans >= 63:
                        assert raw[3].max() > g and raw[3].min() < 0
                T = InjectionTables(*raw, nchans)
                got = inject_host(x, T, t_origin, seed=5)
                want = ic.numpy_inject(x, T, t_origin, seed=5)
                assert got.dtype == x.dtype and got.tobytes() == want.tobytes(), (g, t_origin, K, log2bins)
                if K == 0:
                    assert got.tobytes() == x.tobytes()
                elif K >= 3 and g * nchans >= 63:      # (a handful of samples may all round to no change)
                    assert got.tobytes() != x.tobytes()


@pytest.mark.parametrize("dtype", ["uint8", "int8"])
def test_saturation(dtype):
    from riptide_amd.injection import inject_host
    x, cases = ic.saturation_case(dtype)
    info = np.iinfo(dtype)
    for T in cases:
        got = inject_host(x, T, seed=1)
        assert got.tobytes() == ic.numpy_inject(x, T, seed=1).tobytes()
        a = float(T.amp[0])
        if abs(a) > 255:
            assert np.all(got == (info.max if a > 0 else info.min))
        else:
            d = got.astype(np.int32) - x.astype(np.int32)
            assert set(np.unique(d)) <= ({0, 1} if a > 0 else {-1, 0})
            assert np.all(got[x == (info.max if a > 0 else info.min)] == (info.max if a > 0 else info.min))


@pytest.mark.parametrize("dtype", ic.DTYPES)
def test_gulp_independence(dtype):
    """The whole block equals two overlapping pieces with their t_origin."""
    from riptide_amd.injection import inject_host
    g, n = 257, 65
    x = ic.block(g, n, dtype)
    T = ic.tables(3, n, g, 1000, 10)
    whole = inject_host(x, T, 1000, seed=9)
    a = inject_host(x[:150], T, 1000, seed=9)
    b = inject_host(x[120:], T, 1120, seed=9)
    assert np.array_equal(a, whole[:150]) and np.array_equal(b, whole[120:])


def _constant_tables(nchans, value):
    from riptide_amd.engine import INJECT_SPEC_DTYPE
    from riptide_amd.injection import InjectionTables
    specs = np.zeros(1, dtype=INJECT_SPEC_DTYPE)
    specs[0]["log2bins"], specs[0]["step"], specs[0]["span"] = 1, 999, ic.SPAN
    return InjectionTables(specs, np.ones(2, dtype=np.float32), np.full(nchans, value, dtype=np.float32),
                           np.zeros(nchans, dtype=np.int32), nchans)


def test_dither():
    """No signal: unchanged.  A constant acc = 0.25 over 2^16 samples: the
    increments are 0 or 1 and their mean is 0.25 within 4 standard errors of
    the binomial, sqrt(0.25 * 0.75 / n) = 0.0017 (seed 2024 gives 0.250076).
    Two seeds differ."""
    from riptide_amd.injection import inject_host
    n = 1 << 16
    x = np.full((256, 256), 100, dtype=np.uint8)
    empty = ic.tables(0, 256, 256, 0, 1)
    assert np.array_equal(inject_host(x, empty, seed=3), x)
    T = _constant_tables(256, 0.25)
    d = inject_host(x, T, seed=2024).astype(np.int64) - 100
    assert set(np.unique(d)) == {0, 1}
    print("mean increment:", d.mean())
    assert abs(d.mean() - 0.25) <= 4.0 * np.sqrt(0.25 * 0.75 / n)
    other = inject_host(x, T, seed=2025).astype(np.int64) - 100
    assert not np.array_equal(other, d) and abs(other.mean() - 0.25) < 0.05
    # an exactly zero acc adds nothing whatever the dither
    assert np.array_equal(inject_host(x, _constant_tables(256, 0.0), seed=2024), x)


NORM_NCHANS, NORM_NSAMP = 16, 6000


def _norm_setup(signal, sigma):
    from riptide_amd.dedispersion import dispersion_delays
    from riptide_amd.injection import injection_tables
    freqs = dc.band(NORM_NCHANS)
    delays, max_delay = dispersion_delays(freqs, [signal.dm], dc.TSAMP)
    span = NORM_NSAMP - max_delay
    return freqs, delays, max_delay, span, injection_tables(signal, freqs, dc.TSAMP, span, sigma)


@pytest.mark.parametrize("what", ["pulsar", "accelerated", "steep", "pulse"])
def test_normalisation(what):
    """Zero float32 data, injected and dedispersed on the host at the true DM:
    sqrt(sum s^2) / sqrt(sum sigma_c^2) is the requested snr to 1e-5 relative
    (float32 amplitudes: 6e-8 each; the sums here are float64)."""
    from riptide_amd.dedispersion import dedisperse_host
    from riptide_amd.injection import PulsarSignal, PulseSignal, inject_host
    sig = {"pulsar": PulsarSignal(0.25, 20.0, 15.0),
           "accelerated": PulsarSignal(0.25, 20.0, 15.0, ducy=0.05, accel=2.0e7, phi0=0.1),
           "steep": PulsarSignal(0.1, 10.0, 40.0, spectral_index=-2.0, log2bins=12),
           "pulse": PulseSignal(2.0, 20.0, 12.0, 0.004, spectral_index=1.0)}[what]
    sigma = np.linspace(1.0, 3.0, NORM_NCHANS)
    freqs, delays, max_delay, span, T = _norm_setup(sig, sigma)
    if what == "accelerated":
        assert 0.1 < abs(float(T.specs[0]["factor"])) * span < 1.0
    x = inject_host(np.zeros((NORM_NSAMP, NORM_NCHANS), dtype=np.float32), T)
    series = dedisperse_host(x, delays, max_delay)[0].astype(np.float64)
    assert series.size == span
    got = np.sqrt(np.sum(series ** 2)) / np.sqrt(np.sum(sigma ** 2))
    print(what, "snr", got)
    assert abs(got - sig.snr) <= 1e-5 * sig.snr
    w = T.amp.astype(np.float64)
    assert np.all(w > 0)
    if what == "steep":
        assert np.allclose(w / w.sum(), (freqs / freqs.mean()) ** -2.0 / np.sum((freqs / freqs.mean()) ** -2.0),
                           rtol=1e-6)


def test_exact_recovery():
    """Amplitudes and template values that are multiples of 2^-6: every
    float32 product and sum is exact, so the series dedispersed at the
    signal's DM is (sum_c amp_c) * tmpl[bin(t)], exactly.  bin(t) is worked
    out here in Python's unbounded integers, sample by sample."""
    from riptide_amd.dedispersion import dedisperse_host, dispersion_delays
    from riptide_amd.engine import INJECT_SPEC_DTYPE
    from riptide_amd.injection import InjectionTables, inject_host
    n, g = 16, 3000
    rng = np.random.RandomState(4)
    delays, max_delay = dispersion_delays(dc.band(n), [30.0], dc.TSAMP)
    span, step, phase0, factor = g - max_delay, (1 << 64) // 137, 12345 << 40, 3e-5
    specs = np.zeros(1, dtype=INJECT_SPEC_DTYPE)
    specs[0]["log2bins"], specs[0]["step"], specs[0]["phase0"] = 6, step, phase0
    specs[0]["factor"], specs[0]["span"] = factor, span
    tmpl = (rng.randint(0, 65, size=64) / 64.0).astype(np.float32)
    amp = (rng.randint(1, 65, size=n) / 64.0).astype(np.float32)
    T = InjectionTables(specs, tmpl, amp, delays[0].astype(np.int32), n)
    x = inject_host(np.zeros((g, n), dtype=np.float32), T)
    series = dedisperse_host(x, delays, max_delay)[0]
    bins = [((phase0 + (t + int(np.rint(factor * float(t * (span - t))))) * step) % (1 << 64)) >> 58
            for t in range(span)]
    assert any(int(np.rint(factor * float(t * (span - t)))) for t in range(span))      # the map does shift
    want = np.float32(amp.astype(np.float64).sum()) * tmpl[np.array(bins)]
    assert np.array_equal(series, want) and series.any()


def test_refusals_write_nothing():
    """Every refusal of the specification, through rt_inject_host on raw
    arrays: RT_EINVAL and the block (canary values) untouched."""
    g, n = 9, 5
    base = ic.raw_tables(2, n, g, 0, 4)

    def refused(change, code=0, t_origin=0):
        specs, tmpl, amp, delay = (a.copy() for a in base)
        out = change(specs, tmpl, amp, delay)
        specs, tmpl, amp, delay = out if out is not None else (specs, tmpl, amp, delay)
        x = np.full((g, n), 77, dtype=np.float32 if code == 2 else np.uint8)
        rc = _raw_host(x, specs, tmpl, amp, delay, t_origin, 1, code)
        assert rc == 1 and np.all(x == 77), change.__doc__

    x = np.full((g, n), 77, dtype=np.uint8)
    assert _raw_host(x, *base) == 0 and not np.all(x == 77)

    def set_(index, field, value):
        def change(specs, *_):
            specs[index][field] = value
        return change

    refused(set_(0, "log2bins", 0))
    refused(set_(0, "log2bins", 17))
    refused(set_(1, "length", 0))
    refused(set_(0, "kind", 2))
    refused(set_(0, "reserved", 1))
    refused(set_(0, "span", (1 << 27) + 1))
    for bad in (np.nan, np.inf, -np.inf, 1.0 / ic.SPAN, -1.0 / ic.SPAN, 1.0):
        refused(set_(1, "factor", bad))
    refused(set_(0, "tmpl_off", 1 << 63))
    refused(set_(0, "amp_off", (1 << 64) - 2))
    refused(set_(1, "delay_off", n + 1))

    def poison(which, value):
        def change(specs, tmpl, amp, delay):
            (tmpl if which == "tmpl" else amp)[-1] = value
        return change

    for v in (np.nan, np.inf, -np.inf):
        refused(poison("tmpl", v))
        refused(poison("amp", v))
    refused(lambda s, t, a, d: (s, t[:-1].copy(), a, d))
    refused(lambda s, t, a, d: (s, t, a[:-1].copy(), d))
    refused(lambda s, t, a, d: (s, t, a, d[:-1].copy()))
    refused(lambda *a: None, t_origin=(1 << 31) - g)
    refused(lambda *a: None, code=2, t_origin=(1 << 31) - g)
    for packed in (0x101, 0x102, 0x104, 0x110, 99):
        refused(lambda *a: None, code=packed)
    # the last origin that passes
    x = np.full((g, n), 77, dtype=np.uint8)
    assert _raw_host(x, *base, t_origin=(1 << 31) - g - 1) == 0


def test_python_refusals(tmp_path):
    """The Python layer: tables are checked on construction, channel counts
    must agree, packed files are refused, inject= must be tables."""
    from riptide_amd.dedispersion import dedisperse_filterbank
    from riptide_amd.injection import (InjectionTables, PulsarSignal, inject_filterbank, inject_host,
                                       injection_tables, resolve_inject)
    from riptide_amd.reading import open_filterbank, pack_samples, write_sigproc
    specs, tmpl, amp, delay = ic.raw_tables(2, 5, 9, 0, 4)
    bad = amp.copy()
    bad[0] = np.inf
    with pytest.raises(ValueError, match="amplitude is not finite"):
        InjectionTables(specs, tmpl, bad, delay, 5)
    with pytest.raises(ValueError, match="INJECT_SPEC_DTYPE"):
        InjectionTables(np.zeros(2), tmpl, amp, delay, 5)
    T = InjectionTables(specs, tmpl, amp, delay, 5)
    with pytest.raises(ValueError, match="5 channels"):
        inject_host(np.zeros((9, 6), dtype=np.uint8), T)
    with pytest.raises(ValueError, match="uint8, int8 or float32"):
        inject_host(np.zeros((9, 5), dtype=np.uint16), T)
    with pytest.raises(ValueError, match="2\\^31"):
        inject_host(np.zeros((9, 5), dtype=np.uint8), T, t_origin=(1 << 31) - 9)
    with pytest.raises(ValueError, match="seed"):
        inject_host(np.zeros((9, 5), dtype=np.uint8), T, seed=-1)
    freqs = dc.band(8)
    with pytest.raises(ValueError, match="two samples"):
        injection_tables(PulsarSignal(1e-3, 0.0, 10.0), freqs, 1e-3, 1000, 1.0)
    with pytest.raises(ValueError, match="log2bins"):
        injection_tables(PulsarSignal(0.1, 0.0, 10.0, log2bins=17), freqs, 1e-3, 1000, 1.0)
    with pytest.raises(ValueError, match="below 1"):
        injection_tables(PulsarSignal(0.1, 0.0, 10.0, accel=1e9), freqs, 1e-3, 100000, 1.0)
    x = np.random.RandomState(0).randint(0, 16, size=(64, 8)).astype(np.uint8)
    write_sigproc(str(tmp_path / "p4.fil"), pack_samples(x, 4).ravel(), ic.header(x, nbits=4))
    packed = open_filterbank(str(tmp_path / "p4.fil"))
    T8 = injection_tables(PulsarSignal(0.01, 0.0, 10.0), packed.freqs, packed.tsamp, 64, 1.0)
    for call in (lambda: resolve_inject(T8, packed), lambda: inject_filterbank(packed, T8, str(tmp_path / "o.fil")),
                 lambda: dedisperse_filterbank(packed, [0.0], inject=T8)):
        with pytest.raises(ValueError, match="packed"):
            call()
    assert not os.path.exists(tmp_path / "o.fil")
    plain = open_filterbank(ic.write_filterbank(tmp_path / "u8.fil", x))
    assert resolve_inject(None, plain) is None
    assert resolve_inject(T8, plain) == (T8, 0) and resolve_inject((T8, 7), plain) == (T8, 7)
    with pytest.raises(ValueError, match="InjectionTables"):
        resolve_inject("tables", plain)
    with pytest.raises(ValueError, match="5 channels"):
        resolve_inject(T, plain)


def test_inject_filterbank_host_parts(tmp_path):
    """The header of the injected copy is the source's, key for key and in
    order; the arguments are checked before a device is looked for."""
    from riptide_amd.injection import PulsarSignal, _start_output, inject_filterbank, injection_tables
    from riptide_amd.reading import open_filterbank
    x = np.zeros((40, 8), dtype=np.int8)
    fb = open_filterbank(ic.write_filterbank(tmp_path / "s.fil", x, source_name="J0000+00"))
    # the file the injected gulps are appended to: the source's header, no samples yet
    _start_output(fb, str(tmp_path / "copy.fil"))
    assert os.path.getsize(tmp_path / "copy.fil") == fb.header.bytesize
    with open(tmp_path / "copy.fil", "ab") as f:      # as the gulps are appended
        x.tofile(f)
    back = open_filterbank(str(tmp_path / "copy.fil"))
    assert list(back.header.items()) == list(fb.header.items()) == list(ic.header(x, source_name="J0000+00").items())
    assert back.dtype == np.int8 and back.nsamp == 40 and np.array_equal(back.freqs, fb.freqs)
    T = injection_tables(PulsarSignal(0.01, 0.0, 10.0), fb.freqs, fb.tsamp, 40, 1.0)
    with pytest.raises(ValueError, match="seed"):
        inject_filterbank(fb, T, str(tmp_path / "o.fil"), seed=1 << 64)
    other = injection_tables(PulsarSignal(0.01, 0.0, 10.0), fb.freqs[:4], fb.tsamp, 40, 1.0)
    with pytest.raises(ValueError, match="4 channels"):
        inject_filterbank(fb, other, str(tmp_path / "o.fil"))
    with pytest.raises(ValueError, match="largest delay"):
        inject_filterbank(fb, PulsarSignal(0.01, 5000.0, 10.0), str(tmp_path / "o.fil"), sigma=1.0)
    assert not os.path.exists(tmp_path / "o.fil")


def test_asan_inject_check():
    """`make asan` builds build/asan/inject_check (g++, AddressSanitizer +
    UBSan, no HIP): rt_inject_check and rt_inject_host on exact-size heap
    arrays over the shapes of this file, pieces against the whole, and every
    error return with nothing written."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "inject_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("inject_check OK")
