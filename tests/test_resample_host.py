"""CPU-only tests of the acceleration search's resampling: the host
specification (rt_resample_host, resample_host.hpp) against the numpy
restatement acceleration.resample_indices at every shape the GPU tests use,
its refusals, the trial grid, the clustering of AccelPeak, the sharded
dispatcher on two fake ranks, the accelerated pulse train through the oracle
periodogram, and the sanitizer build of the checker."""
import os
import socket
import subprocess

import numpy as np
import pytest

import resample_common as rc
from conftest import REPO


@pytest.fixture(scope="module")
def ac():
    from riptide_amd import acceleration
    return acceleration


@pytest.mark.parametrize("n", rc.SIZES)
def test_host_equals_numpy_restatement(ac, n):
    x, names, fs, out = rc.host_case(n)
    assert out.shape == (2 * len(fs), n) and out.dtype == np.float32
    for b in range(2):
        for k, (name, f) in enumerate(zip(names, fs)):
            ref = x[b, ac.resample_indices(n, f)]
            assert np.array_equal(rc.bits(out[b * len(fs) + k]), rc.bits(ref)), (n, name)
    # f = 0 and the tiny factors are the identity
    for k in (names.index("zero"), names.index("tiny+"), names.index("tiny-")):
        assert np.array_equal(rc.bits(out[k]), rc.bits(x[0]))
    if n >= 3:
        assert ac.resample_indices(n, -rc.edge_factor(n))[n - 1] == n - 1       # clamped from n


@pytest.mark.parametrize("B,R,N", rc.BATCH_SHAPES)
def test_batch_shapes_strides_and_values(ac, B, R, N):
    """src repeated, permuted and leaving sources unused; rows of a wider
    array with NaN in the gaps are read in place."""
    src, f = rc.batch_rows(B, R, N)
    x = rc.series(B, N, 50 + B, ld=N + 5)
    out = ac.resample_host(x, f, src=src)
    for r in range(R):
        assert np.array_equal(rc.bits(out[r]), rc.bits(x[src[r], ac.resample_indices(N, f[r])])), r
    assert not np.any(np.isnan(out))
    if B == 5:
        assert 1 not in src and len(set(src.tolist())) == min(4, R)


def test_special_values_are_copied_bitwise(ac):
    x = rc.special_values()
    f = [0.0, rc.edge_factor(x.shape[1]), -0.37 * rc.edge_factor(x.shape[1])]
    out = ac.resample_host(x, f)
    for k, ff in enumerate(f):
        assert np.array_equal(rc.bits(out[k]), rc.bits(x[0])[ac.resample_indices(x.shape[1], ff)])
    assert np.array_equal(rc.bits(out[0]), rc.bits(x[0]))


def test_default_rows_and_empty_calls(ac):
    x = rc.series(3, 100, 1)
    f = [0.0, 1e-3, -2e-3]
    out = ac.resample_host(x, f)
    src, ff = ac.resample_rows(3, f)
    assert src.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2] and ff.tolist() == f * 3
    assert np.array_equal(out, ac.resample_host(x, ff, src=src))
    assert ac.resample_host(x, []).shape == (0, 100)
    assert ac.resample_host(np.zeros((2, 0), dtype=np.float32), [0.0]).shape == (2, 0)
    assert ac.resample_host(x[0], [0.0]).shape == (1, 100)


def test_refusals(ac):
    from riptide_amd import _lib
    L = _lib.load()
    x = rc.series(2, 64, 2)
    with pytest.raises(ValueError, match=r"\|factor\| \* N must be below 1"):
        ac.resample_host(x, [1.0 / 64.0])
    with pytest.raises(ValueError, match=r"\|factor\| \* N must be below 1"):
        ac.resample_host(x, [0.0, -1.0 / 64.0])
    assert ac.resample_host(x, [np.nextafter(1.0 / 64.0, 0.0)]).shape == (2, 64)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="not finite"):
            ac.resample_host(x, [bad])
    for src in ([2], [-1], [1 << 40]):
        with pytest.raises(ValueError, match=r"source row outside \[0, B\)"):
            ac.resample_host(x, [0.0], src=src)
    with pytest.raises(ValueError, match="one entry per output row"):
        ac.resample_host(x, [0.0, 0.0], src=[0])
    with pytest.raises(ValueError, match="float32"):
        ac.resample_host(x.astype(np.float64), [0.0])
    # what the wrapper cannot be made to pass: straight to the entry point
    src, f, out = np.zeros(1, dtype=np.int32), np.zeros(1), np.zeros((1, 64), dtype=np.float32)

    def call(xp, N, ldx, sp, fp, R, op, ldo):
        return L.rt_resample_host(xp, 2, N, ldx, sp, fp, R, op, ldo)
    P = _lib.ptr
    assert call(P(x), 64, 64, P(src), P(f), 1, P(out), 64) == _lib.RT_OK
    for args, msg in [((P(x), 64, 63, P(src), P(f), 1, P(out), 64), "input row stride below"),
                      ((P(x), 64, 64, P(src), P(f), 1, P(out), 63), "output row stride below"),
                      ((None, 64, 64, P(src), P(f), 1, P(out), 64), "null pointer"),
                      ((P(x), 64, 64, None, P(f), 1, P(out), 64), "null pointer"),
                      ((P(x), 64, 64, P(src), None, 1, P(out), 64), "null pointer"),
                      ((P(x), 64, 64, P(src), P(f), 1, None, 64), "null pointer"),
                      ((P(x), (1 << 27) + 1, 1 << 28, P(src), P(f), 1, P(out), 1 << 28), "more than 2\\^27 samples"),
                      ((P(x), 64, 64, P(src), P(f), 65536, P(out), 64), "more than 65535 rows")]:
        with pytest.raises(ValueError, match=msg):
            _lib.check(call(*args))
    # nothing to do: no pointer is looked at
    assert call(None, 64, 0, None, None, 0, None, 0) == _lib.RT_OK
    assert call(None, 0, 0, None, None, 3, None, 0) == _lib.RT_OK


def test_accel_factor_and_trials(ac):
    assert ac.C == 299792458.0
    # 50 m/s^2 at 64 us: 50 * 64e-6 / (2 * 299792458) = 5.3370255...e-12, by hand
    assert ac.accel_factor(50.0, 64e-6) == pytest.approx(5.337025e-12, rel=1e-6)
    assert ac.accel_factor(50.0, 64e-6) == 50.0 * 64e-6 / 599584916.0
    assert ac.accel_factor(-3.0, 1e-3) == -ac.accel_factor(3.0, 1e-3) and ac.accel_factor(0.0, 1e-3) == 0.0
    # T = 600 s, a = 50 m/s^2: the drift a T^2 / (8 c) is 7.5 ms, so a step that leaves `smear` is 16 c smear / T^2
    assert 50.0 * 600.0 ** 2 / (8 * ac.C) == pytest.approx(7.505e-3, rel=1e-3)
    assert ac.accel_step(600.0, 1e-3) == pytest.approx(16 * 299792458.0 * 1e-3 / 360000.0)
    half = ac.accel_step(600.0, 1e-3) / 2
    assert half * 600.0 ** 2 / (8 * ac.C) == pytest.approx(1e-3)
    for amax, tobs, smear in [(50.0, 600.0, 1e-3), (500.0, 600.0, 1e-4), (5.0, 600.0, 1e-3), (0.0, 600.0, 1e-3),
                              (1234.5, 65.536, 2.5e-3)]:
        t = ac.accel_trials(amax, tobs, smear)
        assert t.dtype == np.float64 and t.size % 2 == 1 and t[t.size // 2] == 0.0 and 0.0 in t.tolist()
        assert np.array_equal(t, -t[::-1]) and np.all(np.diff(t) > 0)
        assert t[0] == -amax and t[-1] == amax
        if t.size > 1:
            assert np.diff(t).max() <= ac.accel_step(tobs, smear)
    assert ac.accel_trials(50.0, 600.0, 1e-3).tolist() == [-50.0, -37.5, -25.0, -12.5, 0.0, 12.5, 25.0, 37.5, 50.0]
    with pytest.raises(ValueError):
        ac.accel_trials(-1.0, 600.0, 1e-3)
    with pytest.raises(ValueError):
        ac.accel_trials(50.0, 600.0, 0.0)


def test_accel_peak_and_clustering(ac):
    import riptide_amd
    from riptide_amd import Peak
    from riptide_amd.clustering import cluster_peaks
    assert riptide_amd.acceleration is ac and callable(riptide_amd.search_filterbank_accel)
    assert ac.AccelPeak._fields == Peak._fields + ("accel",)
    plain = [Peak(0.5, 2.0, 3, 0.01, 1, 10, 9.0, 5.0), Peak(0.25, 4.0, 3, 0.01, 1, 20, 8.0, 5.0),
             Peak(0.5001, 1 / 0.5001, 3, 0.01, 1, 11, 12.0, 10.0), Peak(1.0, 1.0, 3, 0.01, 1, 30, 7.5, 5.0)]
    acc = [ac.AccelPeak(*p, a) for p, a in zip(plain, (0.0, 10.0, -10.0, 10.0))]
    assert acc[0].summary_dict()["accel"] == 0.0 and set(acc[0].summary_dict()) == set(plain[0].summary_dict()) | {"accel"}
    ps, cl = ac.cluster_peaks([tuple(p) for p in acc], 0.2, 100.0)
    rps, rcl = cluster_peaks(plain, 0.2, 100.0)
    assert [p[:8] for p in ps] == [tuple(p) for p in rps]
    assert [[p[:8] for p in c] for c in cl] == [[tuple(p) for p in c] for c in rcl]
    assert sorted(len(c) for c in cl) == [1, 1, 2] and all(isinstance(p, ac.AccelPeak) for p in ps)
    assert ac.cluster_peaks([], 0.2, 100.0) == ([], [])


# ---------------------------------------------------------------- the accelerated pulse train, on the CPU

def test_oracle_periodogram_prefers_the_true_acceleration(ac, oracle):
    """resample_host + the oracle periodogram on the series of the GPU test:
    within one cluster radius of 2 Hz the trial at the true acceleration has
    the highest S/N of the five, above the trial at zero."""
    x = rc.accel_series()
    rows = ac.resample_host(x, [ac.accel_factor(a, rc.ACC_TSAMP) for a in rc.ACC_TRIALS])
    kw = rc.ACC_RANGES[0]["ffa_search"]
    widths = oracle.generate_width_trials(kw["bins_min"], 0.2)
    best = []
    for row in rows:
        periods, _, snrs = oracle.periodogram(oracle.normalise(row), rc.ACC_TSAMP, widths, kw["period_min"],
                                              kw["period_max"], kw["bins_min"], kw["bins_max"])
        near = rc.near_signal(1.0 / periods)
        assert near.sum() > 3
        best.append(float(snrs[near].max()))
    print("best S/N per trial:", dict(zip(rc.ACC_TRIALS, best)))
    assert int(np.argmax(best)) == rc.ACC_TRIALS.index(rc.ACC_A)
    assert best[3] > best[2]


# ---------------------------------------------------------------- the dispatcher on two fake ranks

class _FakeFilterbank:
    """What dispatch.search_filterbank_accel asks of a Filterbank."""


class _FakeSearcher:
    """EngineSearcher.search_filterbank_accel's contract without a GPU: per
    DM, one peak per acceleration and `range`, carrying nout in ip."""

    def search_filterbank_accel(self, fb, dms, accels, mask=None, nout=None, kdm=None, zero_dm=False,
                                block_mask=None):
        from riptide_amd.acceleration import AccelPeak
        return [[AccelPeak(0.5 + k, 1.0 / (0.5 + k), 3, 0.01, 1, int(nout), 9.0, dm, a) for a in accels
                 for k in range(2)] for dm in dms]


def _fake_fb(path):
    from riptide_amd.reading import Filterbank, write_sigproc
    x = np.random.RandomState(5).randint(0, 256, size=(3000, 8)).astype(np.uint8)
    header = {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": 1e-3, "nbits": 8,
              "fch1": 400.0, "foff": -4.0, "nchans": 8, "nifs": 1}
    write_sigproc(str(path), x, header)
    return Filterbank(str(path))


FAKE_DMS = [0.0, 30.0, 10.0, 50.0, 20.0, 40.0, 5.0]
FAKE_ACCELS = [-3.0, 0.0, 3.0]


def _accel_worker(rank, world, port, fname, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import riptide_amd
        peaks = riptide_amd.search_filterbank_accel(fname, FAKE_DMS, FAKE_ACCELS, _FakeSearcher())
        q.put((rank, [tuple(p) for p in peaks]))
    finally:
        dist.destroy_process_group()


def test_search_filterbank_accel_order_and_two_ranks(ac, tmp_path):
    import torch.multiprocessing as mp
    import riptide_amd
    from riptide_amd.dedispersion import dispersion_delays
    fb = _fake_fb(tmp_path / "fake.fil")
    single = riptide_amd.search_filterbank_accel(fb, FAKE_DMS, FAKE_ACCELS, _FakeSearcher(), group=None)
    assert all(isinstance(p, ac.AccelPeak) for p in single)
    # in the order of dms, then accels, then range
    assert [(p.dm, p.accel, p.period) for p in single] == [(dm, a, 0.5 + k) for dm in FAKE_DMS for a in FAKE_ACCELS
                                                           for k in range(2)]
    # every series is cut to what the whole DM list leaves
    _, max_delay = dispersion_delays(fb.freqs, FAKE_DMS, fb.tsamp)
    assert max_delay > 0 and {p.ip for p in single} == {fb.nsamp - max_delay}
    assert riptide_amd.search_filterbank_accel(fb, [], FAKE_ACCELS, _FakeSearcher()) == []
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_accel_worker, args=(r, 2, port, fb.fname, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert results[0] == results[1] == [tuple(p) for p in single]


def test_asan_resample_check():
    """`make asan` builds build/asan/resample_check (g++, AddressSanitizer +
    UBSan, no HIP): rt_resample_host on exact-size heap arrays at every size
    and edge factor of the GPU tests, and every error return."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "resample_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("resample_check OK")
