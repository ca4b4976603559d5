"""GPU tests of the resampling kernel (csrc/resample_kernels.hip) and the
acceleration search built on it.  engine.resample_device is compared bit for
bit (uint32 views) with the host specification rt_resample_host, which
test_resample_host.py pins to its numpy restatement; the searches are compared
field for field with the same steps done by hand."""
import numpy as np
import pytest

import dedisp_common as dc
import resample_common as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def engine():
    from riptide_amd import engine
    return engine


@pytest.fixture(scope="module")
def ac():
    from riptide_amd import acceleration
    return acceleration


@pytest.mark.parametrize("n", rc.SIZES)
def test_device_equals_host_bit_for_bit(torch, engine, n):
    """Every size with every factor of its case: zero, the tiny factors, the
    ties at N = 1025, the edge factors (the negative one reaches the upper
    clamp) and a random one."""
    x, names, fs, ref = rc.host_case(n)
    got = engine.resample_device(torch.from_numpy(np.ascontiguousarray(x)).cuda(), fs).cpu().numpy()
    assert got.shape == ref.shape
    for r in range(ref.shape[0]):
        assert np.array_equal(rc.bits(got[r]), rc.bits(ref[r])), (n, names[r % len(names)])


@pytest.mark.parametrize("B,R,N", rc.BATCH_SHAPES)
def test_batch_shapes_strides_and_canaries(torch, engine, ac, B, R, N):
    """src repeated, permuted and leaving sources unused (300 rows: three
    launches); the input rows of a wider tensor with NaN in the gaps; output
    rows of a wider tensor whose gaps must survive, once starting on a 16-byte
    boundary and once at an odd float offset (the 4-byte store path)."""
    src, f = rc.batch_rows(B, R, N)
    x = rc.series(B, N, 50 + B, ld=N + 5)
    ref = ac.resample_host(x, f, src=src)
    wide = torch.from_numpy(np.ascontiguousarray(x.base if x.base is not None else x)).cuda()
    assert wide.shape == (B, N + 5)
    xd = wide[:, :N]
    for off, ld in ((0, N + 11), (3, N + 8)):
        canvas = torch.full((R, off + ld), -12345.0, dtype=torch.float32, device="cuda")
        out = canvas[:, off:off + N]
        assert out.data_ptr() % 16 == 4 * off
        got = engine.resample_device(xd, f, src=src, out=out)
        assert got.data_ptr() == out.data_ptr()
        host = canvas.cpu().numpy()
        assert np.array_equal(rc.bits(host[:, off:off + N]), rc.bits(ref)), (off, ld)
        assert np.all(host[:, :off] == -12345.0) and np.all(host[:, off + N:] == -12345.0)


def test_side_stream_and_special_values(torch, engine, ac):
    """NaN payloads, infinities, -0.0 and denormals are copied bitwise; the
    call is ordered on the stream it is given."""
    x = rc.special_values()
    f = [0.0, rc.edge_factor(x.shape[1]), -0.37 * rc.edge_factor(x.shape[1])]
    ref = ac.resample_host(x, f)
    side = torch.cuda.Stream()
    xd = torch.from_numpy(x.copy()).cuda()
    side.wait_stream(torch.cuda.current_stream())
    got = engine.resample_device(xd, f, stream=side)
    side.synchronize()
    assert np.array_equal(rc.bits(got.cpu().numpy()), rc.bits(ref))
    # a 1-D series, and the default rows of a batch
    one = engine.resample_device(xd[0], f[1:2])
    assert tuple(one.shape) == (1, x.shape[1]) and np.array_equal(rc.bits(one.cpu().numpy()), rc.bits(ref[1:2]))
    y = rc.series(3, 257, 9)
    got = engine.resample_device(torch.from_numpy(np.ascontiguousarray(y)).cuda(), [0.0, 1e-3, -2e-3])
    assert np.array_equal(rc.bits(got.cpu().numpy()), rc.bits(ac.resample_host(y, [0.0, 1e-3, -2e-3])))
    assert tuple(engine.resample_device(xd, []).shape) == (0, x.shape[1])


def test_refusals_launch_nothing(torch, engine):
    x = torch.zeros((2, 64), dtype=torch.float32, device="cuda")
    out = torch.full((1, 64), 7.0, dtype=torch.float32, device="cuda")

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            engine.resample_device(*args, out=kw.pop("out", out), **kw)
    refused(r"\|factor\| \* N must be below 1", x, [1.0 / 64.0], src=[0])
    refused(r"\|factor\| \* N must be below 1", x, [-1.0 / 64.0], src=[1])
    for bad in (np.nan, np.inf, -np.inf):
        refused("not finite", x, [bad], src=[0])
    for src in ([2], [-1], [1 << 40]):
        refused(r"source row outside \[0, B\)", x, [0.0], src=src)
    refused("one entry per output row", x, [0.0, 0.0], src=[0])
    refused("out must be", x, [0.0], src=[0], out=torch.zeros((1, 63), dtype=torch.float32, device="cuda"))
    refused("out must be", x, [0.0], src=[0], out=torch.zeros((1, 64), dtype=torch.float64, device="cuda"))
    refused("output row stride below", x, [0.0, 0.0], src=[0, 1],
            out=torch.zeros(128, dtype=torch.float32, device="cuda").as_strided((2, 64), (32, 1)))
    refused("input row stride below", torch.zeros(128, dtype=torch.float32, device="cuda").as_strided((2, 64), (32, 1)),
            [0.0], src=[0])
    refused("data must be", x.double(), [0.0], src=[0])
    refused("more than 65535 rows", x, np.zeros(65536), src=np.zeros(65536, dtype=np.int32),
            out=torch.empty((65536, 64), dtype=torch.float32, device="cuda"))
    # more than 2^27 samples: allocated, never touched
    big = torch.empty((1, (1 << 27) + 1), dtype=torch.float32, device="cuda")
    refused("more than 2\\^27 samples", big, [0.0], src=[0], out=big)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 7.0)


# ---------------------------------------------------------------- wiring, with no tolerance

WIRE_DEREDDEN = {"rmed_width": 2.0, "rmed_minpts": 101}
WIRE_RANGES = [{"name": "a", "ffa_search": {"period_min": 0.1, "period_max": 0.5, "bins_min": 64, "bins_max": 72,
                                            "ducy_max": 0.1}, "find_peaks": {"smin": 5.0}},
               {"name": "b", "ffa_search": {"period_min": 0.5, "period_max": 2.0, "bins_min": 64, "bins_max": 72,
                                            "ducy_max": 0.1}, "find_peaks": {"smin": 5.0}}]


def test_search_device_accel_equals_the_steps_by_hand(torch, engine, ac):
    """[3, 2^14] with accels [-a, 0, a]: the peaks of every (trial, accel)
    equal those of deredden_normalise -> resample_host on the CPU -> upload ->
    the searcher's own plan and finder, field for field, accel attached."""
    import inputs
    from riptide_amd.dispatch import EngineSearcher
    n, tsamp, a = 1 << 14, 1e-3, 4e5              # shifts of up to a N^2 tsamp / (8 c) = 45 samples
    raw = np.stack([inputs.with_signal(n, tsamp, 300 + k, 0.17 + 0.21 * k, 30.0) for k in range(3)])
    accels = [-a, 0.0, a]
    metas = [{"dm": 10.0 * k} for k in range(3)]
    searcher = EngineSearcher(WIRE_DEREDDEN, WIRE_RANGES, device=0, batch=4)
    rawd = torch.from_numpy(raw).cuda()
    got = searcher.search_device_accel(rawd, tsamp, metas, accels)
    assert len(got) == 3 and sum(len(g) for g in got) > 0
    x = engine.deredden_normalise(rawd, int(round(WIRE_DEREDDEN["rmed_width"] / tsamp)), WIRE_DEREDDEN["rmed_minpts"])
    rows = ac.resample_host(x.cpu().numpy(), [ac.accel_factor(v, tsamp) for v in accels])
    rowsd = torch.from_numpy(rows).cuda()
    want = [[] for _ in range(3)]
    for r0 in range(0, 9, searcher.batch):          # the (trial, accel) rows, trial-major, in the searcher's slices
        rows_of = list(range(r0, min(r0 + searcher.batch, 9)))
        found = [[] for _ in rows_of]
        for conf in WIRE_RANGES:
            plan = searcher._plan(n, tsamp, conf)
            snr = plan.run(rowsd[rows_of[0]:rows_of[-1] + 1])
            finder = searcher._finder(plan, n * tsamp, conf)
            for i, (peaks, _) in enumerate(finder(snr, dms=[metas[r // 3]["dm"] for r in rows_of])):
                found[i].extend(peaks)
        for r, peaks in zip(rows_of, found):
            want[r // 3].extend(ac.AccelPeak(*p, accels[r % 3]) for p in peaks)
    assert [[tuple(p) for p in g] for g in got] == [[tuple(p) for p in w] for w in want]
    assert {p.accel for g in got for p in g} == set(accels)
    assert all(p.dm == metas[k]["dm"] for k in range(3) for p in got[k])
    # no trial accelerations, no series
    assert searcher.search_device_accel(rawd, tsamp, metas, []) == [[], [], []]
    assert searcher.search_device_accel(rawd[:0], tsamp, [], accels) == []


E2E_DMS = [0.0, 10.0, 20.0, 30.0, 40.0]
E2E_DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}
E2E_RANGES = [{"name": "short",
               "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
               "find_peaks": {"smin": 7.0}}]


def test_search_filterbank_accel_at_zero_equals_search_filterbank(torch, ac, tmp_path):
    """accels = [0.0] on a small 8-bit file: search_filterbank's peaks with
    accel == 0.0, in the order of dms; the searcher's method returns one list
    per DM."""
    import riptide_amd
    from riptide_amd.dispatch import EngineSearcher
    from riptide_amd.reading import Filterbank, write_sigproc
    nchans, nsamp = 16, 1 << 15
    rng = np.random.RandomState(4321)
    x = rng.normal(100.0, 10.0, size=(nsamp, nchans))
    sweep = dc.numpy_delays(dc.band(nchans), [20.0], dc.TSAMP)[0]
    for c in range(nchans):
        for t0 in range(100 + int(sweep[c]), nsamp - 8, 500):
            x[t0:t0 + 8, c] += 6.0
    header = {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": dc.TSAMP, "nbits": 8,
              "fch1": 400.0, "foff": -32.0 / nchans, "nchans": nchans, "nifs": 1}
    write_sigproc(str(tmp_path / "s.fil"), np.clip(np.round(x), 0, 255).astype(np.uint8), header)
    fb = Filterbank(str(tmp_path / "s.fil"))
    searcher = EngineSearcher(E2E_DEREDDEN, E2E_RANGES, device=0, batch=2)
    ref = riptide_amd.search_filterbank(fb, E2E_DMS, searcher)
    got = riptide_amd.search_filterbank_accel(fb, E2E_DMS, [0.0], searcher, group=None)
    assert len(ref) > 0 and all(isinstance(p, ac.AccelPeak) and p.accel == 0.0 for p in got)
    assert [tuple(p)[:8] for p in got] == [tuple(p) for p in ref]
    dms = [p.dm for p in got]
    assert dms == sorted(dms) and max(ref, key=lambda p: p.snr).dm == 20.0
    per_dm = searcher.search_filterbank_accel(fb, E2E_DMS[:3], [0.0, 100.0])
    assert len(per_dm) == 3 and all({p.dm for p in plist} <= {dm} for dm, plist in zip(E2E_DMS, per_dm))
    for plist in per_dm:
        assert [p.accel for p in plist] == sorted(p.accel for p in plist)      # accel order within a DM


# ---------------------------------------------------------------- the point of it all

def test_accelerated_pulsar_is_found_at_its_acceleration(torch, ac):
    """The pulse train of resample_common (drift of four pulse widths at
    mid-observation) searched over [-2a, -a, 0, a, 2a]: the brightest peak
    within one cluster radius of 2 Hz has accel == a and beats the best peak
    of the accel = 0 trial there.  (The same ordering on the CPU:
    test_resample_host.py, the oracle periodogram.)"""
    from riptide_amd.dispatch import EngineSearcher
    x = torch.from_numpy(rc.accel_series()).cuda()[None, :]
    searcher = EngineSearcher(rc.ACC_DEREDDEN, rc.ACC_RANGES, device=0, batch=4)
    peaks, = searcher.search_device_accel(x, rc.ACC_TSAMP, [{"dm": 0.0}], rc.ACC_TRIALS)
    near = [p for p in peaks if rc.near_signal(p.freq)]
    assert near
    best = max(near, key=lambda p: p.snr)
    at_zero = max([p.snr for p in near if p.accel == 0.0], default=0.0)
    print("best:", best, "best at accel 0:", at_zero)
    assert best.accel == rc.ACC_A
    assert best.snr > at_zero
    # the trials of the signal fall into one cluster, whose brightest member is the same peak
    _, clusters = ac.cluster_peaks(peaks, rc.ACC_RADIUS, rc.ACC_TOBS)
    mine = [c for c in clusters if best in c]
    assert len(mine) == 1 and max(mine[0], key=lambda p: p.snr) == best


def test_time_series_resample(torch, ac):
    from riptide_amd import TimeSeries
    accel = 40 * rc.ACC_A                  # shifts of up to 15 of the 4099 samples
    ts = TimeSeries(rc.accel_series()[:4099], rc.ACC_TSAMP, metadata={"dm": 3.0})
    out = ts.resample(accel)
    assert out.metadata["accel"] == accel and out.metadata["dm"] == 3.0 and "accel" not in ts.metadata
    assert out.tsamp == ts.tsamp and out.nsamp == ts.nsamp
    ref = ac.resample_host(ts.data, [ac.accel_factor(accel, rc.ACC_TSAMP)])[0]
    assert np.array_equal(rc.bits(out.data), rc.bits(ref)) and not np.array_equal(out.data, ts.data)
