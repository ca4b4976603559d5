"""CPU-only tests of the candidate-building stage: the fold's shape rules and
argument validation through the C ABI (nothing is launched: every device
pointer is null), PeakCluster, Candidate and get_search_range."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import inputs


@pytest.fixture(scope="module")
def lib():
    from riptide_amd import _lib
    return _lib.load()


def _shape(lib, size, factor, bins, subints):
    m, rows = ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib.rt_fold_shape(size, factor, bins, subints or 0, ctypes.byref(m), ctypes.byref(rows))
    return rc, m.value, rows.value


def _ref_rows(m, subints):
    """folding.py:64-81: rows of the result, 0 for a 1-D profile."""
    if subints == 1 or m == 1:
        return 0
    if subints is None or subints == m:
        return m
    vf = m / subints
    return int(np.floor(m / vf))         # downsample.hpp:21-24 on the m rows


def test_fold_shape_matches_reference_rules(lib):
    quirks = 0
    for m in range(1, 301):
        # n = floor(size / 2) = 2 m (+ 1: a dropped partial period), bins = 2
        for size in (4 * m, 4 * m + 3):
            for subints in [None] + list(range(1, m + 1)):
                rc, gm, rows = _shape(lib, size, 2.0, 2, subints)
                assert rc == 0, (m, subints, lib.rt_last_error())
                assert gm == m
                want = _ref_rows(m, subints)
                assert rows == want, (m, subints, rows, want)
                if subints not in (None, 1, m) and m > 1 and want == subints - 1:
                    quirks += 1
    assert quirks > 0, "no (m, subints) pair with floor(m / (m / subints)) == subints - 1 was seen"
    assert _ref_rows(9, 7) == 6 and _shape(lib, 36, 2.0, 2, 7) == (0, 9, 6)
    # m == 1: a profile whatever subints says
    for subints in (None, 1):
        assert _shape(lib, 4, 2.0, 2, subints) == (0, 1, 0)
    # another factor / bins: m = floor(floor(1000 / 1.7) / 13)
    assert _shape(lib, 1000, 1.7, 13, None) == (0, 45, 45)
    assert _shape(lib, 1000, 1.7, 13, 45) == (0, 45, 45)
    assert _shape(lib, 1000, 1.7, 13, 1) == (0, 45, 0)


def _specs(rows):
    from riptide_amd.folding import FOLD_SPEC
    t = np.zeros(len(rows), dtype=FOLD_SPEC)
    for k, r in enumerate(rows):
        t[k] = (r["factor"], r.get("out_off", 0), r.get("series", 0), r["bins"], r.get("subints", 0), 0)
    return t


def test_fold_spec_layout():
    from riptide_amd.folding import FOLD_SPEC
    assert FOLD_SPEC.itemsize == 32
    assert [FOLD_SPEC.fields[n][1] for n in ("factor", "out_off", "series", "bins", "subints", "reserved")] == \
        [0, 8, 16, 20, 24, 28]


SIZE = 4096
GOOD = dict(factor=4.0, bins=16)      # m = 64, rows result: 1024 floats

EINVAL_CASES = {
    "factor_one": ([dict(GOOD, factor=1.0)], 1, 1 << 20),
    "factor_below_one": ([dict(GOOD, factor=0.5)], 1, 1 << 20),
    "factor_above_size": ([dict(GOOD, factor=SIZE + 0.5)], 1, 1 << 20),
    "factor_nan": ([dict(GOOD, factor=float("nan"))], 1, 1 << 20),
    "bins_one": ([dict(GOOD, bins=1)], 1, 1 << 20),
    "bins_zero": ([dict(GOOD, bins=0)], 1, 1 << 20),
    "no_whole_period": ([dict(factor=400.0, bins=16)], 1, 1 << 20),          # n = 10 < bins
    "subints_above_m": ([dict(GOOD, subints=65)], 1, 1 << 20),
    "series_out_of_range": ([dict(GOOD, series=2)], 2, 1 << 20),
    "output_past_end": ([dict(GOOD, out_off=1)], 1, 1024),
    "output_offset_past_end": ([dict(GOOD, subints=1, out_off=1 << 40)], 1, 1024),
    "outputs_overlap": ([dict(GOOD, out_off=0), dict(GOOD, subints=1, out_off=1023)], 1, 1 << 20),
    "second_spec_bad": ([dict(GOOD), dict(GOOD, bins=1, out_off=1024)], 1, 1 << 20),
}


@pytest.mark.parametrize("name", sorted(EINVAL_CASES))
def test_fold_rejects_bad_arguments_without_launching(lib, name):
    from riptide_amd._lib import RT_EINVAL, ptr
    rows, nseries, out_floats = EINVAL_CASES[name]
    t = _specs(rows)
    rc = lib.rt_fold_device(None, SIZE, SIZE, nseries, ptr(t), len(t), None, out_floats, None, 1 << 30, None)
    assert rc == RT_EINVAL, name
    assert lib.rt_last_error()
    rc = lib.rt_fold(None, SIZE, nseries, ptr(t), len(t), None, out_floats)
    assert rc == RT_EINVAL, name
    assert lib.rt_last_error()


def test_fold_rejects_short_workspace_and_accepts_no_specs(lib):
    from riptide_amd._lib import RT_EINVAL, RT_OK, ptr
    t = _specs([dict(GOOD, subints=4, out_off=0), dict(GOOD, out_off=64)])
    need = ctypes.c_size_t()
    assert lib.rt_fold_workspace_bytes(SIZE, ptr(t), len(t), ctypes.byref(need)) == RT_OK
    assert need.value >= 1024 * 4          # the first spec's row array lives in the workspace
    rc = lib.rt_fold_device(None, SIZE, SIZE, 1, ptr(t), len(t), None, 64 + 1024, None, need.value - 1, None)
    assert rc == RT_EINVAL and b"workspace" in lib.rt_last_error()
    bad = _specs([dict(GOOD, bins=1)])
    assert lib.rt_fold_workspace_bytes(SIZE, ptr(bad), 1, ctypes.byref(need)) == RT_EINVAL
    assert lib.rt_fold_device(None, SIZE, SIZE, 1, None, 0, None, 0, None, 0, None) == RT_OK
    assert lib.rt_fold(None, SIZE, 1, None, 0, None, 0) == RT_OK
    assert lib.rt_fold_workspace_bytes(SIZE, None, 0, ctypes.byref(need)) == RT_OK and need.value == 0


def test_check_fold_args_messages():
    from riptide_amd.folding import check_fold_args
    assert check_fold_args(10.0, 1e-3, 1.0, 100, None) == (1.0 / 100 / 1e-3, None)
    assert check_fold_args(10.0, 1e-3, 1.0, 100, 2.0)[1] == 2
    with pytest.raises(ValueError, match="Period exceeds data length"):
        check_fold_args(10.0, 1e-3, 1e6, 100, None)
    with pytest.raises(ValueError, match="Bin width is shorter than sampling time"):
        check_fold_args(10.0, 1e-3, 1.0, 10 ** 6, None)
    with pytest.raises(ValueError, match="subints must be >= 1 or None"):
        check_fold_args(10.0, 1e-3, 1.0, 100, 0)
    with pytest.raises(ValueError, match="exceeds the number of signal periods"):
        check_fold_args(10.0, 1e-3, 1.0, 100, 10 ** 6)


class _Series:
    """What fold()'s argument checks read of a TimeSeries (they raise before
    any data is touched)."""

    def __init__(self, nsamp, tsamp):
        self.nsamp, self.tsamp = nsamp, tsamp
        self.length = nsamp * tsamp
        self.data = None


BAD_FOLD_ARGS = [(1e6, 100, None), (1.0, 10 ** 6, None), (1e-6, 100, None), (1.0, 100, 0), (1.0, 100, -3),
                 (1.0, 100, 10 ** 6), (1.0, 100, 11), (1.0, 100, 11.9)]


@pytest.mark.parametrize("period,bins,subints", BAD_FOLD_ARGS)
def test_check_fold_args_raises_what_fold_raises(period, bins, subints):
    """The batched paths validate with check_fold_args: the same exception
    text as fold() itself for the same bad arguments."""
    from riptide_amd.folding import check_fold_args, fold, fold_many
    ts = _Series(10000, 1e-3)
    with pytest.raises(ValueError) as want:
        fold(ts, period, bins, subints)
    with pytest.raises(ValueError) as got:
        check_fold_args(ts.length, ts.tsamp, period, bins, subints)
    assert str(got.value) == str(want.value)
    ts.data = np.zeros(ts.nsamp, np.float32)
    with pytest.raises(ValueError) as many:
        fold_many(ts, [(period, bins, subints)])
    assert str(many.value) == str(want.value)


def test_no_whole_period_is_rejected_before_the_batched_call():
    """period == series length passes fold()'s checks and can still leave
    floor(nsamp / factor) < bins: candidate_fold_spec raises, so that
    build_candidates leaves the cluster out."""
    from riptide_amd import PeakCluster
    from riptide_amd.candidate import candidate_fold_spec
    from riptide_amd.folding import check_fold_args
    ts = _Series(1007, 1e-3)
    period, bins = ts.length, 128
    factor, _ = check_fold_args(ts.length, ts.tsamp, period, bins, None)
    assert int(np.floor(ts.nsamp / factor)) < bins
    confs = [{"ffa_search": {"period_min": 0.1, "period_max": 10.0}, "candidates": {"bins": bins, "subints": 4}}]
    with pytest.raises(ValueError, match="no whole period"):
        candidate_fold_spec(ts, PeakCluster([_peak(period, 9.0, 0.0)]), confs)
    assert candidate_fold_spec(ts, PeakCluster([_peak(0.2, 9.0, 0.0)]), confs) == (0.2, bins, 4)
    assert candidate_fold_spec(ts, PeakCluster([_peak(0.5, 9.0, 0.0)]), confs) == (0.5, bins, None)


def _peak(period, snr, dm, width=3, bins=100, iw=1, ip=7):
    from riptide_amd import Peak
    return Peak(period=period, freq=1.0 / period, width=width, ducy=width / bins, iw=iw, ip=ip, snr=snr, dm=dm)


def test_peak_cluster_centre_and_summary():
    from riptide_amd import PeakCluster
    peaks = [_peak(1.0, 9.0, 0.0), _peak(1.0001, 21.5, 10.0), _peak(0.9999, 12.0, 20.0)]
    cl = PeakCluster(peaks, rank=3)
    assert cl.centre is peaks[1] and len(cl) == 3 and not cl.is_harmonic
    d = cl.summary_dict()
    assert list(d) == ["period", "freq", "dm", "width", "ducy", "snr", "npeaks", "rank", "hfrac_num", "hfrac_denom",
                       "fundamental_rank"]
    assert d["period"] == 1.0001 and d["snr"] == 21.5 and d["dm"] == 10.0 and d["npeaks"] == 3
    # a fundamental: integer defaults, its own rank as the fundamental's
    assert (d["rank"], d["hfrac_num"], d["hfrac_denom"], d["fundamental_rank"]) == (3, 0, 0, 3)
    fundamental = PeakCluster([_peak(2.0, 40.0, 10.0)], rank=0)
    h = PeakCluster(peaks, rank=3, parent_fundamental=fundamental, hfrac=Fraction(4, 2))
    d = h.summary_dict()
    assert h.is_harmonic
    assert (d["rank"], d["hfrac_num"], d["hfrac_denom"], d["fundamental_rank"]) == (3, 2, 1, 0)
    assert "size=3" in str(cl) and repr(cl) == str(cl)
    assert PeakCluster([]).rank is None


def test_peak_cluster_dataframes():
    pytest.importorskip("pandas")
    from riptide_amd import PeakCluster
    from riptide_amd.peak_cluster import clusters_to_dataframe
    a = PeakCluster([_peak(1.0, 9.0, 0.0), _peak(1.0, 11.0, 10.0)], rank=1)
    b = PeakCluster([_peak(3.0, 30.0, 10.0)], rank=0)
    df = a.summary_dataframe()
    assert list(df.columns) == ["period", "freq", "dm", "width", "ducy", "snr"] and len(df) == 2
    assert list(df.snr) == [9.0, 11.0]
    table = clusters_to_dataframe([a, b])
    assert list(table.columns) == ["rank", "period", "dm", "snr", "ducy", "freq", "npeaks", "hfrac_num",
                                   "hfrac_denom", "fundamental_rank"]
    assert list(table.snr) == [30.0, 11.0] and list(table["rank"]) == [0, 1]
    assert table.hfrac_num.dtype.kind == "i" and table.fundamental_rank.dtype.kind == "i"


def test_candidate_round_trip_and_profile():
    from riptide_amd import Candidate
    sub = np.random.RandomState(3).normal(size=(4, 16)).astype(np.float32)
    c = Candidate({"period": 1.0, "snr": 12.0}, {"dm": 5.0}, "peaks", sub)
    d = c.to_dict()
    assert set(d) == {"params", "tsmeta", "peaks", "subints"}
    c2 = Candidate.from_dict(d)
    assert c2.params is c.params and c2.tsmeta is c.tsmeta and c2.peaks == "peaks" and c2.subints is sub
    assert np.array_equal(c.profile, sub.sum(axis=0))
    flat = Candidate({"snr": 1.0}, {}, None, sub[0])
    assert flat.profile is flat.subints
    assert str(c) == "Candidate({'period': 1.0, 'snr': 12.0})" and repr(c) == str(c)


def test_candidate_dm_curve():
    pytest.importorskip("pandas")
    from riptide_amd import Candidate, PeakCluster
    cl = PeakCluster([_peak(1.0, 9.0, 0.0), _peak(1.0, 11.0, 10.0), _peak(1.0, 10.0, 10.0, width=5)])
    c = Candidate(cl.summary_dict(), {}, cl.summary_dataframe(), np.zeros(8, np.float32))
    dm, snr = c.dm_curve
    assert list(dm) == [0.0, 10.0] and list(snr) == [9.0, 11.0]


class _StubSeries:
    """Records what Candidate.from_pipeline_output asks of TimeSeries.fold."""

    def __init__(self, length):
        self.length = length
        self.metadata = {"dm": 10.0, "tobs": length}
        self.calls = []

    def fold(self, period, bins, subints=None):
        self.calls.append((period, bins, subints))
        return np.zeros(bins, np.float32)


def test_from_pipeline_output_subints_rule():
    pytest.importorskip("pandas")       # Candidate.peaks is the cluster's DataFrame
    from riptide_amd import Candidate, PeakCluster
    cl = PeakCluster([_peak(2.0, 15.0, 10.0), _peak(2.5, 9.0, 0.0)], rank=0)
    ts = _StubSeries(64.0)
    c = Candidate.from_pipeline_output(ts, cl, 128, subints=16)        # 16 x 2 s < 64 s: passed through
    c1 = Candidate.from_pipeline_output(ts, cl, 128)                   # default: one sub-integration
    Candidate.from_pipeline_output(ts, cl, 128, subints=32)            # 32 x 2 s >= 64 s: None
    Candidate.from_pipeline_output(ts, cl, 128, subints=64)
    Candidate.from_pipeline_output(ts, cl, 128, subints=None)
    assert ts.calls == [(2.0, 128, 16), (2.0, 128, 1), (2.0, 128, None), (2.0, 128, None), (2.0, 128, None)]
    # params: the centre peak's six fields, not the cluster summary (candidate.py:98)
    assert c.params == {"period": 2.0, "freq": 0.5, "dm": 10.0, "width": 3, "ducy": 3 / 100, "snr": 15.0}
    assert list(c.params) == ["period", "freq", "dm", "width", "ducy", "snr"] and c.tsmeta is ts.metadata
    assert len(c.peaks) == 2 and c.subints.shape == (128,) and c1.params["snr"] == 15.0


def test_get_search_range():
    from riptide_amd.candidate import get_search_range
    ranges = [dict(r, candidates={"bins": 128 * (k + 1), "subints": 32}) for k, r in
              enumerate(inputs.PIPELINE_CASE["ranges"])]
    shuffled = ranges[::-1]
    for confs in (ranges, shuffled):
        assert get_search_range(confs, 0.1)["name"] == "medium"        # below the global minimum: the first
        assert get_search_range(confs, 0.5)["name"] == "medium"
        assert get_search_range(confs, 3.999)["name"] == "medium"
        assert get_search_range(confs, 4.0)["name"] == "long"          # period_min inclusive, period_max not
        assert get_search_range(confs, 119.0)["name"] == "long"
        assert get_search_range(confs, 120.0)["name"] == "long"        # at the global maximum: the last
        assert get_search_range(confs, 500.0)["name"] == "long"
    got = get_search_range(ranges, 1.0)
    assert got == ranges[0] and got is not ranges[0]                   # a copy
    assert got["candidates"]["bins"] == 128


def test_modules_import_no_plotting_and_pandas_only_in_functions():
    import ast
    import riptide_amd.candidate
    import riptide_amd.peak_cluster
    for mod in (riptide_amd.candidate, riptide_amd.peak_cluster):
        tree = ast.parse(open(mod.__file__).read())
        everywhere, top = set(), set()
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                everywhere |= {a.name.split(".")[0] for a in node.names}
            elif isinstance(node, ast.ImportFrom) and node.module and not node.level:
                everywhere.add(node.module.split(".")[0])
        for node in tree.body:
            if isinstance(node, ast.Import):
                top |= {a.name.split(".")[0] for a in node.names}
            elif isinstance(node, ast.ImportFrom) and node.module and not node.level:
                top.add(node.module.split(".")[0])
        assert not everywhere & {"matplotlib", "astropy"}, mod.__name__
        assert "pandas" not in top, mod.__name__
