"""CPU-only tests of the dedispersion front end: the delay table
(rt_dedisperse_delays) against the numpy evaluation of its formula, the host
specification (rt_dedisperse_host) against the numpy restatement, the
Filterbank reader, and the sanitizer program.  No call reaches the GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dedisp_common as dc
from conftest import REPO

NCHANS = (1, 3, 37, 64, 65)
DMS = (0.0, 50.0, 12.5, 50.0, 3.0)


@pytest.fixture(scope="module")
def lib():
    from riptide_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("ascending", [False, True])
@pytest.mark.parametrize("nchans", NCHANS)
def test_delay_table(nchans, ascending):
    from riptide_amd.dedispersion import KDM, dispersion_delays
    assert KDM == 1.0 / 2.41e-4
    freqs = dc.band(nchans, ascending)
    delays, max_delay = dispersion_delays(freqs, DMS, dc.TSAMP)
    ref = dc.numpy_delays(freqs, DMS, dc.TSAMP)
    assert delays.dtype == np.int64 and delays.shape == (len(DMS), nchans)
    assert np.array_equal(delays, ref)
    assert max_delay == ref.max()
    assert not delays[0].any()                      # DM 0
    assert np.array_equal(delays[1], delays[3])     # equal DMs
    assert delays[:, np.argmax(freqs)].max() == 0   # the reference channel
    # another constant and sampling time
    d2, m2 = dispersion_delays(freqs, DMS, 64e-6, kdm=4.148808e3)
    assert np.array_equal(d2, dc.numpy_delays(freqs, DMS, 64e-6, 4.148808e3)) and m2 == d2.max()


def test_delay_table_errors(lib):
    from riptide_amd import _lib
    from riptide_amd.dedispersion import dispersion_delays
    f = dc.band(4)
    cases = [
        (([], [1.0], 1e-3), "nchans and ndm"),
        ((f, [], 1e-3), "nchans and ndm"),
        (([400.0, 0.0], [1.0], 1e-3), "frequencies must be positive and finite"),
        (([400.0, -1.0], [1.0], 1e-3), "frequencies must be positive and finite"),
        (([400.0, np.inf], [1.0], 1e-3), "frequencies must be positive and finite"),
        (([400.0, np.nan], [1.0], 1e-3), "frequencies must be positive and finite"),
        ((f, [-0.5], 1e-3), "DMs must be non-negative and finite"),
        ((f, [np.nan], 1e-3), "DMs must be non-negative and finite"),
        ((f, [np.inf], 1e-3), "DMs must be non-negative and finite"),
        ((f, [1.0], 0.0), "tsamp must be > 0"),
        ((f, [1.0], -1e-3), "tsamp must be > 0"),
        ((f, [1.0], 1e-16), "2^31"),
    ]
    for args, text in cases:
        with pytest.raises(ValueError, match=text.replace("^", r"\^")):
            dispersion_delays(*args)
    # the return code itself
    fr = np.array([400.0, 390.0])
    dm = np.array([-1.0])
    out = np.zeros(2, dtype=np.int64)
    md = ctypes.c_int64()
    assert lib.rt_dedisperse_delays(_lib.ptr(fr), 2, _lib.ptr(dm), 1, 1e-3, 1.0, _lib.ptr(out),
                                    ctypes.byref(md)) == _lib.RT_EINVAL
    assert b"DMs" in lib.rt_last_error()
    # just below 2^31 is accepted, max_delay may be NULL
    dm[0] = 1.0
    a = 1.0 / (390.0 * 390.0) - 1.0 / (400.0 * 400.0)
    tsamp = a / 2147483000.0
    assert lib.rt_dedisperse_delays(_lib.ptr(fr), 2, _lib.ptr(dm), 1, tsamp, 1.0, _lib.ptr(out), None) == _lib.RT_OK
    assert out[0] == 0 and out[1] == int(np.floor(1.0 * 1.0 * a / tsamp + 0.5)) < 2 ** 31


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.float32])
@pytest.mark.parametrize("nchans", NCHANS)
def test_host_specification(nchans, dtype):
    from riptide_amd.dedispersion import dedisperse_host, dispersion_delays
    rng = np.random.RandomState(nchans)
    for ascending in (False, True):
        delays, max_delay = dispersion_delays(dc.band(nchans, ascending), DMS, dc.TSAMP)
        nsamp = max_delay + 257
        x = dc.samples(rng, nsamp, nchans, dtype)
        masks = [None]
        if nchans >= 3:
            m = np.zeros(nchans, dtype=bool)
            m[[0, nchans - 1]] = True
            only = np.ones(nchans, dtype=bool)
            only[nchans // 2] = False
            masks += [m, only]
        for mask in masks:
            for nout in (nsamp - max_delay, 1):   # the last output reads the last sample; a single output
                out = dedisperse_host(x, delays, max_delay, mask=mask, nout=nout)
                dc.assert_dedispersed(out, x, delays, nout, mask)
        # masking never changes the alignment: the table has no mask argument
        with pytest.raises(ValueError, match="nout \\+ max_delay exceeds"):
            dedisperse_host(x, delays, max_delay, nout=nsamp - max_delay + 1)


def test_host_specification_errors():
    from riptide_amd.dedispersion import dedisperse_host
    x = np.ones((10, 2), dtype=np.uint8)
    d = np.array([[0, 3]], dtype=np.int64)
    assert dedisperse_host(x, d, 3)[0, -1] == 2.0
    with pytest.raises(ValueError, match="outside \\[0, max_delay\\]"):
        dedisperse_host(x, d, 2, nout=1)
    with pytest.raises(ValueError, match="outside \\[0, max_delay\\]"):
        dedisperse_host(x, -d, 3)
    with pytest.raises(ValueError, match="uint8, int8 or float32"):
        dedisperse_host(x.astype(np.int16), d, 3)
    with pytest.raises(ValueError, match="one entry per channel"):
        dedisperse_host(x, d, 3, mask=[True])


def test_workspace_bytes(lib):
    """Host-only: rows padded to 16 bytes; NULL and bad shapes are RT_EINVAL."""
    from riptide_amd import _lib
    b = ctypes.c_size_t()
    assert lib.rt_dedisperse_workspace_bytes(0, 1001, 37, ctypes.byref(b)) == _lib.RT_OK and b.value == 1008 * 37
    assert lib.rt_dedisperse_workspace_bytes(2, 1001, 37, ctypes.byref(b)) == _lib.RT_OK and b.value == 4016 * 37
    assert lib.rt_dedisperse_workspace_bytes(0, 1001, 37, None) == _lib.RT_EINVAL
    assert b"NULL" in lib.rt_last_error()
    assert lib.rt_dedisperse_workspace_bytes(5, 1001, 37, ctypes.byref(b)) == _lib.RT_EINVAL
    assert lib.rt_dedisperse_workspace_bytes(1, 1001, 65794, ctypes.byref(b)) == _lib.RT_EINVAL
    assert lib.rt_dedisperse_workspace_bytes(2, 1001, 65794, ctypes.byref(b)) == _lib.RT_OK


def _header(nchans, nbits, foff, **extra):
    h = {"telescope_id": 4, "machine_id": 10, "data_type": 1, "source_name": "J0000-0000", "src_raj": 123456.7,
         "src_dej": -123456.7, "tstart": 59000.5, "tsamp": 256e-6, "nbits": nbits, "fch1": 400.0 if foff < 0 else 368.0,
         "foff": foff, "nchans": nchans, "nifs": 1}
    h.update(extra)
    return h


@pytest.mark.parametrize("dtype,extra", [(np.uint8, {}), (np.uint8, {"signed": False}), (np.int8, {"signed": True}),
                                         (np.float32, {})])
@pytest.mark.parametrize("foff", [-0.5, 0.5])
def test_filterbank_round_trip(tmp_path, dtype, extra, foff):
    import riptide_amd
    from riptide_amd.reading import Filterbank, write_sigproc
    assert riptide_amd.Filterbank is Filterbank
    nchans, nsamp = 37, 501
    x = dc.samples(np.random.RandomState(5), nsamp, nchans, dtype)
    header = _header(nchans, 8 * np.dtype(dtype).itemsize, foff, **extra)
    fname = str(tmp_path / "fb.fil")
    write_sigproc(fname, x, header)
    fb = Filterbank(fname)
    assert (fb.nsamp, fb.nchans, fb.tsamp) == (nsamp, nchans, 256e-6)
    assert fb.dtype == np.dtype(dtype)
    assert np.array_equal(fb.freqs, header["fch1"] + np.arange(nchans) * foff) and fb.freqs.dtype == np.float64
    assert isinstance(fb.data, np.memmap) and fb.data.shape == (nsamp, nchans) and not fb.data.flags.writeable
    assert np.array_equal(fb.data, x)
    for key, val in header.items():
        assert fb.header[key] == val
    meta = fb.metadata(dm=12.5)
    assert isinstance(meta, riptide_amd.Metadata)
    assert meta["dm"] == 12.5 and meta["source_name"] == "J0000-0000" and meta["mjd"] == 59000.5
    assert meta["tobs"] == nsamp * 256e-6 and meta["fname"] == os.path.realpath(fname)
    assert meta["skycoord"] == fb.header.skycoord
    # the time series reader still refuses the file, with its own message
    with pytest.raises(ValueError, match="contains multi-channel data"):
        riptide_amd.TimeSeries.from_sigproc(fname)


def test_filterbank_errors(tmp_path):
    from riptide_amd.reading import Filterbank, write_sigproc
    x = np.zeros((16, 4), dtype=np.uint8)
    fname = str(tmp_path / "bad.fil")
    write_sigproc(fname, x, _header(4, 8, -1.0, nifs=2))
    with pytest.raises(ValueError, match="nifs = 2"):
        Filterbank(fname)
    for nbits, arr in ((16, x.astype(np.uint16)), (4, x), (2, x), (1, x)):
        if nbits == 16:
            write_sigproc(fname, arr, _header(4, 16, -1.0))
        else:
            write_sigproc(fname, arr.ravel(), _header(4, nbits, -1.0))
        with pytest.raises(ValueError, match=f"contains {nbits}-bit data"):
            Filterbank(fname)
    with pytest.raises(ValueError, match="nchans must equal"):
        write_sigproc(fname, x, _header(5, 8, -1.0))
    with pytest.raises(ValueError, match="nbits must equal"):
        write_sigproc(fname, x, _header(4, 32, -1.0))


def test_sanitizer_program():
    """`make asan` builds build/asan/dedisp_check (g++, AddressSanitizer +
    UBSan, no HIP): rt_dedisperse_delays and rt_dedisperse_host on exact-size
    heap arrays over the edge shapes and every error return."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "dedisp_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("dedisp_check OK")


# ------------------------------------------- the sum kernel's staging rule
def test_span_plan_table():
    """engine.dedisperse_span_plan (rt_dedisperse_span_plan: dedisp_span of
    dedisp_types.hpp, the rule dedisp_sum_kernel itself calls) against the
    closed forms, for both element sizes, every lo % 4 and every spread from 0
    to past both thresholds: 8-bit rows are staged iff hi - (lo & ~3) <= 800,
    float rows iff hi - lo <= 264, and the full spans of 264 and 520 dwords are
    reached exactly."""
    from riptide_amd import engine
    seen = {1: set(), 4: set()}
    for lo in (0, 1, 2, 3, 4, 5, 6, 7, 1000, 1001, 1002, 1003, 2 ** 31 - 1300):
        for spread in list(range(0, 12)) + list(range(255, 275)) + list(range(790, 810)):
            hi = lo + spread
            ndw, staged = engine.dedisperse_span_plan(1, lo, hi)
            w8 = hi - (lo & ~3)
            assert ndw == (256 + w8 + 3) // 4 and staged == (w8 <= 800), (lo, hi, ndw, staged)
            assert staged == (ndw <= dc.SPAN_DWORDS[1])
            seen[1].add((ndw, staged))
            ndw, staged = engine.dedisperse_span_plan(4, lo, hi)
            assert ndw == 256 + spread and staged == (spread <= 264), (lo, hi, ndw, staged)
            assert staged == (ndw <= dc.SPAN_DWORDS[4])
            seen[4].add((ndw, staged))
    assert {(264, True), (265, False)} <= seen[1] and {(520, True), (521, False)} <= seen[4]
    # the last staged spread hi - lo of 8-bit rows: 800, 799, 798, 797 by lo % 4
    for r in range(4):
        assert engine.dedisperse_span_plan(1, 8 + r, 8 + r + 800 - r) == (264, True)
        assert engine.dedisperse_span_plan(1, 8 + r, 8 + r + 801 - r) == (265, False)
    assert dc.LAST_STAGED == {1: 4 * dc.SPAN_DWORDS[1] - dc.TIME_TILE, 4: dc.SPAN_DWORDS[4] - dc.TIME_TILE}
    assert engine.dedisperse_span_plan(1, 0, 2 ** 31 - 1) == ((256 + 2 ** 31 - 1 + 3) // 4, False)
    for bad in ((0, 0, 1), (2, 0, 1), (8, 0, 1), (-1, 0, 1), (1, 5, 4), (4, 5, 4), (1, -1, 4), (4, -3, -2),
                (1, 0, 2 ** 31), (4, -2 ** 31, 0)):
        with pytest.raises(ValueError, match="span_plan"):
            engine.dedisperse_span_plan(*bad)


def test_path_tables():
    """The preconditions of dedisp_common's hand-made delay tables, on numpy
    and the span plan alone: what the GPU path tests rely on is a property of
    their inputs."""
    tables = dc.path_tables()
    assert {"mixed", "residues", "clamp"} <= set().union(*(t[4] for t in tables.values()))
    for name, (delays, mask, max_delay, esize, claims) in tables.items():
        assert delays.dtype == np.int64 and delays.ndim == 2, name
        assert delays.shape[1] <= 40 and delays.shape[0] <= 33 and max_delay + 300 <= 1500, name
        inside = (delays >= 0) & (delays <= max_delay)
        if "clamp" in claims:
            wild = delays[~inside]
            assert {-1, -2 ** 31, max_delay + 1, 2 ** 31 - 1} == set(int(v) for v in wild), name
            assert np.abs(delays).max() < 2 ** 31 + 1 and delays.min() >= -2 ** 31      # the table fits int32
            paths = dc.tile_paths(delays, max_delay, esize)
            hit = (~inside).any(axis=0)
            assert "S" in paths[0, hit] and "D" in paths[0, hit], name
        else:
            assert inside.all(), name
        paths = dc.tile_paths(delays, max_delay, esize, mask)
        if name.startswith("threshold"):
            # class S channels sit exactly at the last staged span, D one sample past it
            from riptide_amd import engine
            clipped = delays[:dc.DM_TILE]
            for c in range(delays.shape[1]):
                ndw, staged = engine.dedisperse_span_plan(esize, clipped[:, c].min(), clipped[:, c].max())
                cls = dc.THRESHOLD_CLASSES[c % len(dc.THRESHOLD_CLASSES)]
                assert (ndw, staged) == ((dc.SPAN_DWORDS[esize], True) if cls == "S" else
                                         (dc.SPAN_DWORDS[esize] + 1, False)), (name, c)
                assert clipped[0, c] == clipped[:, c].min() and clipped[-1, c] == clipped[:, c].max()
            assert len(set(int(v) % 4 for v in clipped.min(axis=0))) == 1
            # the partial step of four channels holds both paths
            assert {"S", "D"} <= set(paths[0, dc.CHAN_STEP:dc.CHAN_STEP + 4]), name
            if delays.shape[0] > dc.DM_TILE:
                assert set(paths[1]) <= {"S", "M"}, name
        if "mixed" in claims:
            assert mask is not None and {"S", "D", "M"} <= set(paths[0, :dc.CHAN_STEP]), name
        if "residues" in claims:
            assert esize == 1 and set(paths.ravel()) == {"S"}, name
            first = delays[:dc.DM_TILE]
            lo = first.min(axis=0)
            pairs = {(int(l) & 3, int(v - l) & 3) for row in first for v, l in zip(row, lo)}
            assert len(pairs) == 16, name
            # a full step of 16 channels alone holds them all, and reads at every byte residue p & 3
            step = {(int(l) & 3, int(v - (l & ~3)) & 3) for row in first for v, l in zip(row[:16], lo[:16])}
            assert len(step) == 16, name


BAND_TABLE = np.array([[0, 20], [3, 19], [16, 20], [15, 17], [9, 9], [11, 13]], dtype=np.uint32)


@pytest.mark.parametrize("kind", ["float32", "u16", "uint8-zero_dm", "int8-zero_dm", "u4-zero_dm"])
def test_float32_restatement_equals_the_host_specification(kind):
    """dc.numpy_dedisperse_f32 -- a float32 accumulator from +0.0, one float32
    addition per unmasked channel in ascending order, under the zero-DM filter
    of float32(x) - m -- has the bits of dedisperse_host and
    dedisperse_bands_host on the hand-made tables: the GPU tests' float
    reference does not rest on the project's C++."""
    from riptide_amd.dedispersion import dedisperse_bands_host, dedisperse_host
    kind, _, zero_dm = kind.partition("-")
    for name in ("threshold-e4-r1-ndm17", "threshold-e4-r2-ndm5", "residues-20ch"):
        delays, mask, max_delay, _, _ = dc.path_tables()[name]
        nout = 70
        x, vals, nbits = dc.kind_samples(np.random.RandomState(len(name)), max_delay + nout, delays.shape[1], kind)
        for m in (None, mask) if mask is not None else (None,):
            mean = dc.numpy_zero_dm_mean(vals, m) if zero_dm else None
            if zero_dm:
                from riptide_amd.dedispersion import zero_dm_mean_host
                assert np.array_equal(mean.view(np.uint32), zero_dm_mean_host(x, mask=m, nbits=nbits).view(np.uint32))
            host = dedisperse_host(x, delays, max_delay, mask=m, nout=nout, zero_dm=bool(zero_dm), nbits=nbits)
            dc.assert_same_bits(host, dc.numpy_dedisperse_f32(vals, delays, nout, m, mean=mean), f"{name}, plain")
            host = dedisperse_bands_host(x, delays, max_delay, BAND_TABLE, mask=m, nout=nout, zero_dm=bool(zero_dm),
                                         nbits=nbits)
            dc.assert_same_bits(host, dc.numpy_dedisperse_f32(vals, delays, nout, m, bands=BAND_TABLE, mean=mean),
                                f"{name}, bands")
            assert not host[:, 4].any() and not np.signbit(host[:, 4]).any()      # the empty band: +0.0


def test_host_refuses_the_unclipped_table():
    """The device call clamps delays outside [0, max_delay] as it reads them
    (test_gpu_dedisp_paths.py::test_delay_clamp); the host specification
    refuses such a table and takes the clipped one."""
    from riptide_amd.dedispersion import dedisperse_host
    for esize, dtype in ((1, np.uint8), (4, np.float32)):
        wild, max_delay = dc.clamp_table(esize)
        x = dc.samples(np.random.RandomState(esize), max_delay + 10, wild.shape[1], dtype)
        with pytest.raises(ValueError, match="outside \\[0, max_delay\\]"):
            dedisperse_host(x, wild, max_delay)
        assert dedisperse_host(x, np.clip(wild, 0, max_delay), max_delay).shape == (wild.shape[0], 10)
