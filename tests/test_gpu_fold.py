"""The batched device fold (fold_rows_kernel / fold_subints_kernel through
rt_fold_device and rt_fold) against the oracle restatement of
riptide/folding.py:19-81 -- oracle.downsample for rows and columns, numpy's
scale and numpy's sum(axis=0) -- and against folding.fold.  Every comparison
is bit for bit."""
import ctypes

import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import riptide_amd
    return riptide_amd


def series(n, seed, period_samples=97.3):
    """Seeded float32 noise plus a pulse train."""
    x = np.random.RandomState(seed).normal(size=n).astype(np.float32)
    phase = (np.arange(n) / period_samples) % 1.0
    x[phase < 0.05] += np.float32(4.0)
    return x


def oracle_fold(O, data, tsamp, period, bins, subints):
    """folding.py:64-81 over the oracle's strict downsample."""
    factor = period / bins / tsamp
    d = O.downsample(data, factor)
    m = d.size // bins
    ref = d[:m * bins].reshape(m, bins).copy()
    ref *= (m * factor) ** -0.5
    if subints == 1 or m == 1:
        return ref.sum(axis=0)
    if subints is None or subints == m:
        return ref
    cols = np.ascontiguousarray(ref.T)
    return np.ascontiguousarray(np.stack([O.downsample(c, m / subints) for c in cols]).T)


def periods_of(n, f, bins):
    return int(np.floor(n / f)) // bins


def device_fold(rt, data, tsamp, specs):
    import torch
    from riptide_amd import engine
    out = engine.fold_device(torch.from_numpy(np.ascontiguousarray(data)).cuda(), tsamp, specs)
    return [o.cpu().numpy() for o in out]


def check_case(rt, O, data, tsamp, period, bins, subints):
    from riptide_amd.folding import fold
    want = oracle_fold(O, data, tsamp, period, bins, subints)
    got, = device_fold(rt, data, tsamp, [(0, period, bins, subints)])
    assert got.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    host = fold(rt.TimeSeries.from_numpy_array(data, tsamp), period, bins, subints)
    assert host.shape == got.shape and np.array_equal(got, host)
    return got


def test_exact_factor_hits_the_last_sample_clamp(rt, oracle):
    tsamp, n, bins = 2.0 ** -10, 4096, 16
    period = 64 * tsamp
    assert period / bins / tsamp == 4.0
    for subints in (None, 1, 8):
        got = check_case(rt, oracle, series(n, 1), tsamp, period, bins, subints)
    assert got.shape == (8, bins)
    assert check_case(rt, oracle, series(n, 1), tsamp, period, bins, None).shape == (64, bins)   # n % bins == 0


# ds_per_block(f) == floor(4092 / (f + 1)) - 1 is 32 at f = 123 (the last
# staged factor) and 31 just above: the global-window path from there on
FACTOR_CASES = [
    # n, f, bins
    (5000, 1.0001, 64),
    (20000, 1.5, 16),
    (30000, 12.2, 64),         # 256 outputs per block, m * bins = 2432: a partial last block
    (40000, 40.1, 16),         # 98 outputs per block
    (60000, 122.99, 16),
    (60000, 123.0, 16),        # 32 outputs per block: the last staged factor
    (60000, 123.01, 16),       # global windows
    (60000, 700.3, 2),
    (60000, 700.3, 16),        # m = 5: one partial block of 256
]


@pytest.mark.parametrize("n,f,bins", FACTOR_CASES, ids=lambda v: str(v))
def test_factors_across_the_staging_boundary(rt, oracle, n, f, bins):
    data = series(n, 2)
    period = f * bins                       # tsamp = 1
    m = periods_of(n, period / bins / 1.0, bins)
    assert m >= 2
    assert check_case(rt, oracle, data, 1.0, period, bins, None).shape == (m, bins)
    assert check_case(rt, oracle, data, 1.0, period, bins, 1).shape == (bins,)
    if m > 3:
        check_case(rt, oracle, data, 1.0, period, bins, 2)


@pytest.mark.parametrize("bins", [2, 64, 250, 1000])
def test_any_number_of_bins(rt, oracle, bins):
    n, f = 60000, 1.5
    data = series(n, 3)
    period = f * bins
    m = periods_of(n, period / bins, bins)
    assert check_case(rt, oracle, data, 1.0, period, bins, None).shape == (m, bins)
    assert check_case(rt, oracle, data, 1.0, period, bins, 1).shape == (bins,)
    sub = min(16, m - 1)
    assert check_case(rt, oracle, data, 1.0, period, bins, sub).shape[1] == bins


def test_partial_period_is_dropped(rt, oracle):
    n, bins, f = 30000, 64, 12.2
    nd = int(np.floor(n / f))
    assert nd % bins != 0                   # the exact-factor case covers n % bins == 0
    got = check_case(rt, oracle, series(n, 4), 1.0, f * bins, bins, None)
    assert got.shape == (nd // bins, bins)


def test_every_subints_mode(rt, oracle):
    n, bins, f = 30000, 64, 12.2
    data = series(n, 5)
    period = f * bins
    m = periods_of(n, period / bins, bins)
    assert m == 38
    for subints, rows in [(None, m), (1, 0), (m, m), (m - 1, None), (2, 2), (16, None)]:
        got = check_case(rt, oracle, data, 1.0, period, bins, subints)
        if rows == 0:
            assert got.shape == (bins,)
        elif rows is not None:
            assert got.shape == (rows, bins)
        else:
            assert got.shape[0] in (subints, subints - 1)


def test_vertical_quirk_one_row_short(rt, oracle):
    """floor(m / (m / subints)) == subints - 1 at (m, subints) = (9, 7): the
    result has 6 rows, as the reference's."""
    n, bins, f = 7100, 64, 12.2
    period = f * bins
    assert periods_of(n, period / bins, bins) == 9 and int(np.floor(9 / (9 / 7))) == 6
    got = check_case(rt, oracle, series(n, 6), 1.0, period, bins, 7)
    assert got.shape == (6, bins)


def test_single_period(rt, oracle):
    n, bins = 5000, 64
    period = 4990.0                          # just under the series length: m == 1
    assert periods_of(n, period / bins, bins) == 1
    for subints in (None, 1):
        assert check_case(rt, oracle, series(n, 7), 1.0, period, bins, subints).shape == (bins,)


BATCH_N = 30000
BATCH_SPECS = [
    # series, period (tsamp = 1), bins, subints
    (0, 12.2 * 64, 64, None), (1, 12.2 * 64, 64, 1), (2, 12.2 * 64, 64, 16), (0, 12.2 * 64, 64, 38),
    (1, 12.2 * 64, 64, 37), (2, 1.5 * 250, 250, None), (0, 1.5 * 250, 250, 1), (1, 1.5 * 250, 250, 7),
    (2, 123.01 * 16, 16, None), (0, 123.01 * 16, 16, 2), (1, 700.3 * 2, 2, 1), (2, 700.3 * 2, 2, 5),
    (0, 1.0001 * 64, 64, 1), (1, 29000.0, 100, None), (2, 40.1 * 16, 16, 3),
]


@pytest.fixture(scope="module")
def batch(rt):
    data = np.stack([series(BATCH_N, 10 + k, 80.0 + 7 * k) for k in range(3)])
    singles = [device_fold(rt, data[s], 1.0, [(0, p, b, sub)])[0] for s, p, b, sub in BATCH_SPECS]
    return data, singles


def test_batched_call_equals_single_calls(rt, oracle, batch):
    data, singles = batch
    assert len(BATCH_SPECS) >= 12 and {s[0] for s in BATCH_SPECS} == {0, 1, 2}
    got = device_fold(rt, data, 1.0, BATCH_SPECS)
    assert len(got) == len(BATCH_SPECS)
    ndims = set()
    for g, want, spec in zip(got, singles, BATCH_SPECS):
        assert g.shape == want.shape and np.array_equal(g, want), spec
        ndims.add(g.ndim)
    assert ndims == {1, 2}
    # two of them against the oracle directly: another row than 0, both kernels
    for k in (4, 7):
        s, p, b, sub = BATCH_SPECS[k]
        assert np.array_equal(got[k], oracle_fold(oracle, data[s], 1.0, p, b, sub))


def test_batched_call_reversed_with_permuted_offsets(rt, batch):
    import torch
    from riptide_amd import _lib
    from riptide_amd.folding import pack_fold_specs
    data, singles = batch
    L = _lib.load()
    specs = BATCH_SPECS[::-1]
    want = singles[::-1]
    table, shapes, total = pack_fold_specs(BATCH_N, BATCH_N * 1.0, 1.0, specs)
    # results laid out in a shuffled order, 5 floats apart
    order = np.random.RandomState(0).permutation(len(specs))
    off = 3
    for k in order:
        table["out_off"][k] = off
        off += int(np.prod(shapes[k])) + 5
    assert not np.array_equal(np.argsort(table["out_off"]), np.arange(len(specs)))
    d = torch.from_numpy(data).cuda()
    out = torch.full((off,), float("nan"), dtype=torch.float32, device="cuda")
    need = ctypes.c_size_t()
    _lib.check(L.rt_fold_workspace_bytes(BATCH_N, _lib.ptr(table), len(specs), ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    _lib.check(L.rt_fold_device(_lib.ptr(d), BATCH_N, d.stride(0), 3, _lib.ptr(table), len(specs), _lib.ptr(out),
                                out.numel(), _lib.ptr(ws), ws.numel(),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    res = out.cpu().numpy()
    used = np.zeros(off, dtype=bool)
    for k, (shape, w) in enumerate(zip(shapes, want)):
        o = int(table["out_off"][k])
        cnt = int(np.prod(shape))
        assert np.array_equal(res[o:o + cnt].reshape(shape), w), specs[k]
        used[o:o + cnt] = True
    assert np.isnan(res[~used]).all()       # nothing written between the results


def test_no_specs(rt):
    import torch
    from riptide_amd import engine
    from riptide_amd.folding import fold_many
    assert engine.fold_device(torch.zeros(1000, device="cuda"), 1.0, []) == []
    assert fold_many(rt.TimeSeries.from_numpy_array(series(1000, 1), 1.0), []) == []


def test_fold_device_errors(rt):
    import torch
    from riptide_amd import engine
    d = torch.from_numpy(series(10000, 1)).cuda()
    for spec, msg in [((0, 1e6, 100, None), "Period exceeds data length"),
                      ((0, 1000.0, 10 ** 6, None), "Bin width is shorter"),
                      ((0, 1000.0, 100, 0), "subints must be >= 1"),
                      ((0, 1000.0, 100, 10 ** 6), "exceeds the number of signal periods"),
                      ((1, 1000.0, 100, None), "series index"),
                      ((0, 1000.0, 1, None), "bins >= 2")]:
        with pytest.raises(ValueError, match=msg):
            engine.fold_device(d, 1.0, [spec])


def test_fold_many_equals_fold_loop(rt):
    from riptide_amd.folding import fold, fold_many
    ts = rt.TimeSeries.from_numpy_array(series(50000, 8), 1e-3)
    specs = [(0.0973, 32, None), (0.0973, 32, 1), (0.0973, 32, 16), (1.234, 250, 8), (1.234, 250, None),
             (7.5, 1000, 1), (7.5, 1000, 3), (49.0, 64, None),
             (0.5, 1, None), (0.5, 1, 1), (0.5, 1, 10)]           # bins == 1: the host path
    got = fold_many(ts, specs)
    assert len(got) == len(specs)
    for g, (p, b, s) in zip(got, specs):
        want = fold(ts, p, b, s)
        assert g.dtype == np.float32 and g.shape == want.shape and np.array_equal(g, want), (p, b, s)
    assert got[8].shape == (100, 1) and got[9].shape == (1,)
    with pytest.raises(ValueError, match="Period exceeds data length"):
        fold_many(ts, [(0.0973, 32, None), (1e6, 32, None)])


def test_no_whole_period(rt):
    """A period equal to the series length passes fold()'s checks and can
    leave floor(nsamp / factor) < bins: fold() fails on (0 * factor) ** -0.5,
    the batched paths raise the engine's ValueError."""
    import torch
    from riptide_amd import engine
    from riptide_amd.folding import fold, fold_many
    ts = rt.TimeSeries.from_numpy_array(series(1007, 9), 1e-3)
    with pytest.raises(ZeroDivisionError):
        fold(ts, ts.length, 128)
    with pytest.raises(ValueError, match="no whole period"):
        fold_many(ts, [(0.1, 16, None), (ts.length, 128, None)])
    with pytest.raises(ValueError, match="no whole period"):
        engine.fold_device(torch.from_numpy(ts.data).cuda(), ts.tsamp, [(0, ts.length, 128, None)])


def test_time_series_fold_method(rt):
    """riptide/tests/test_time_series.py:160-201 through TimeSeries.fold."""
    from riptide_amd.folding import fold
    length, tsamp, period, bins = 10.0, 1e-3, 1.0, 100
    np.random.seed(0)
    ts = rt.TimeSeries.generate(length, tsamp, period, amplitude=20.0)
    x10 = ts.fold(1.0, bins, subints=None)
    assert x10.shape == (10, bins)
    x2 = ts.fold(1.0, bins, subints=2)
    assert x2.shape == (2, bins)
    m = int(length / period)
    xm = ts.fold(1.0, bins, subints=m)
    prof = ts.fold(1.0, bins, subints=1)
    assert prof.shape == (bins,)
    for other in (x2, x10, xm):
        assert np.allclose(prof, other.sum(axis=0), atol=1.0e-6)    # the reference test's FLOAT_ATOL
    assert np.array_equal(xm, fold(ts, 1.0, bins, subints=m)) and np.array_equal(xm, x10)
    assert np.array_equal(prof, fold(ts, 1.0, bins, subints=1))
    assert np.array_equal(ts.fold(1.0, bins), fold(ts, 1.0, bins))
    for kwargs in (dict(period=1.0, bins=bins, subints=10 ** 6), dict(period=1.0, bins=bins, subints=0),
                   dict(period=1.0, bins=10 ** 6, subints=None), dict(period=1e6, bins=bins, subints=None),
                   dict(period=1e-6, bins=bins, subints=None)):
        with pytest.raises(ValueError):
            ts.fold(**kwargs)


def test_build_candidates(rt):
    import pandas  # noqa: F401  (Candidate.peaks is a DataFrame)
    from riptide_amd import Peak, PeakCluster, build_candidates
    from riptide_amd.candidate import effective_subints
    from riptide_amd.folding import fold
    case = inputs.PIPELINE_CASE
    tobs, tsamp = 16.0, case["tsamp"]                  # 62500 samples
    trials = {dm: rt.TimeSeries.from_numpy_array(
        inputs.generated_series(tobs, tsamp, case["period"], amp, ducy, rt.generate_signal), tsamp)
        for dm, amp, ducy in case["trials"]}
    assert all(ts.nsamp <= 1 << 16 for ts in trials.values())
    for dm, ts in trials.items():
        ts.metadata["dm"] = dm
    confs = [dict(case["ranges"][0], candidates={"bins": 128, "subints": 8}),
             dict(case["ranges"][1], candidates={"bins": 256, "subints": 32})]

    def peak(period, snr, dm, width=3):
        return Peak(period=period, freq=1.0 / period, width=width, ducy=width / 500, iw=1, ip=0, snr=snr, dm=dm)

    clusters = [
        PeakCluster([peak(0.5003, 12.0, 0.0), peak(0.5004, 8.0, 10.0)], rank=2),
        PeakCluster([peak(1.0, 30.0, 10.0), peak(1.0001, 22.0, 0.0), peak(0.9999, 21.0, 20.0)], rank=0),
        PeakCluster([peak(5.0, 9.0, 20.0)], rank=3),               # long range: 32 x 5 s >= 16 s -> None
        PeakCluster([peak(2.0, 18.0, 10.0)], rank=1),
        PeakCluster([peak(3.0, 7.5, 0.0)], rank=4),                # 8 x 3 s >= 16 s -> None
        PeakCluster([peak(20.0, 25.0, 10.0)], rank=5),             # longer than the data: logged, left out
    ]
    loads = []

    def load_series(dm):
        loads.append(dm)
        return trials[dm]

    cands = build_candidates(clusters, load_series, confs, case["dereddening"])
    assert sorted(loads) == [0.0, 10.0, 20.0]                     # once per DM
    assert loads[0] == 10.0                                       # the brightest cluster's DM first
    assert [c.params["snr"] for c in cands] == [30.0, 18.0, 12.0, 9.0, 7.5]
    by_snr = sorted(clusters[:5], key=lambda cl: cl.centre.snr, reverse=True)
    for c, cl in zip(cands, by_snr):
        assert c.params == cl.centre.summary_dict()               # six keys, as the reference's Candidate
        assert list(c.params) == ["period", "freq", "dm", "width", "ducy", "snr"]
    prepared = {dm: ts.deredden(case["dereddening"]["rmed_width"], minpts=case["dereddening"]["rmed_minpts"])
                .normalise() for dm, ts in trials.items()}
    shapes = []
    for c in cands:
        period, dm = c.params["period"], c.params["dm"]
        conf = confs[1 if period >= 4.0 else 0]["candidates"]
        subints = effective_subints(tobs, period, conf["subints"])
        want = fold(prepared[dm], period, conf["bins"], subints)
        assert np.array_equal(c.subints, want), c
        assert c.tsmeta["dm"] == dm and len(c.peaks) == len(by_snr[cands.index(c)])
        shapes.append(c.subints.shape)
    assert shapes[0] == (8, 128) and shapes[3] == (3, 256) and shapes[4] == (5, 128)
    assert build_candidates([], load_series, confs, case["dereddening"]) == []
