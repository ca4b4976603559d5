"""Dereddening and normalisation (rt_deredden_normalise_device: scrunch,
running median, interpolate-and-subtract, normalise) against the oracle's
numpy restatement, at every kernel form and edge of dered_common.CASES and in
every buffer layout of dered_common.LAYOUTS, three different series a call.

The dereddened series equals float32(x - oracle.fast_running_median(x, ws,
mp)) value for value (np.array_equal) in every layout, and bit for bit with
the per-sample interpolation; the interpolated median on its own (scrunch,
running median, np.interp) equals the oracle's too.  The normalised series --
statistics summed by the dereddening kernel, by their own vector or scalar
read passes, in aligned and unaligned buffers -- lies within 2e-6 x
max(|ref|, 1) of oracle.normalise of that series and of every other variant
(DESIGN.md section 3.3).  Nothing outside the output rows is written and the
input is left as it was.
tests/test_host.py::test_dered_cases_cover_the_kernels states which kernel
forms the table reaches."""
import numpy as np
import pytest

import dered_common as dc

pytestmark = pytest.mark.gpu

ENV = ("RIPTIDE_AMD_INTERP_PER_SAMPLE", "RIPTIDE_AMD_NORM_UNFUSED", "RIPTIDE_AMD_NORM_SCALAR")
CASES = {c["name"]: c for c in dc.CASES}
_refs = {}


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import riptide_amd
    return riptide_amd


def refs(oracle, case):
    """(series, dereddened, dereddened + normalised, normalised alone) of a
    case by the oracle, computed once; a series of zero variance normalises
    to NaN, as numpy has it."""
    if case["name"] not in _refs:
        xs = dc.series(case)
        with np.errstate(invalid="ignore", divide="ignore"):
            dered = np.stack([np.asarray(x - oracle.fast_running_median(x, case["ws"], case["mp"]), dtype=np.float32)
                              for x in xs])
            both = np.stack([oracle.normalise(d) for d in dered])
            alone = np.stack([oracle.normalise(x) for x in xs])
        for a in (xs, dered, both, alone):
            a.setflags(write=False)
        _refs[case["name"]] = (xs, dered, both, alone)
    return _refs[case["name"]]


def _buffer(B, n, off, stride):
    """(a flat buffer of SENTINEL, its [B, n] view that starts `off` floats
    past a 16-byte boundary with rows `stride` floats apart)"""
    import torch
    flat = torch.full((B * stride + 8,), dc.SENTINEL, dtype=torch.float32, device="cuda")
    view = flat[off:off + B * stride].view(B, stride)[:, :n]
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off and view.stride(0) == stride
    return flat, view


def run(monkeypatch, case, layout, xs, env=(), **kw):
    """engine.deredden_normalise of the series in a layout with the switches
    of `env` set, as a host array."""
    import torch
    from riptide_amd import engine
    ioff, ooff, istride, ostride = dc.geometry(case, layout)
    B, n = xs.shape
    iflat, x = _buffer(B, n, ioff, istride)
    x.copy_(torch.tensor(xs))
    before = iflat.clone()
    for k in ENV:
        if k in env:
            monkeypatch.setenv(k, "1")
        else:
            monkeypatch.delenv(k, raising=False)
    if ostride is None:
        out = engine.deredden_normalise(x, case["ws"], case["mp"], **kw)
        assert out.data_ptr() % 16 == 0 and out.stride(0) == n
        got = out.cpu().numpy()
    else:
        oflat, out = _buffer(B, n, ooff, ostride)
        engine.deredden_normalise(x, case["ws"], case["mp"], out=out, **kw)
        got = out.cpu().numpy()
        out.fill_(dc.SENTINEL)
        assert bool((oflat == dc.SENTINEL).all()), f"{layout}: written outside the output rows"
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert torch.equal(iflat, before), f"{layout}: the input changed"
    return got


def scaled_error(got, ref, scale, what):
    """max |got - ref| / max(|scale|, 1), NaN allowed only where both have it"""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    err = np.abs(got.astype(np.float64) - ref)[~nan] / np.maximum(np.abs(scale[~nan]), 1.0)
    return float(err.max()) if err.size else 0.0


def assert_variants(outs, ref):
    """every variant within NORM_BOUND x max(|ref|, 1) of the reference and of
    every other variant"""
    names = list(outs)
    for i, a in enumerate(names):
        worst = scaled_error(outs[a], ref, ref, a)
        print(f"{a}: max scaled error vs the oracle {worst:.3e}")
        assert worst <= dc.NORM_BOUND, (a, worst)
        for b in names[i + 1:]:
            d = scaled_error(outs[a], outs[b], ref, (a, b))
            assert d <= dc.NORM_BOUND, (a, b, d)


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_dereddened_equals_oracle(rt, oracle, monkeypatch, name):
    case = CASES[name]
    xs, dered, _, _ = refs(oracle, case)
    outs = {lay: run(monkeypatch, case, lay, xs, normalise=False) for lay in dc.LAYOUTS}
    for lay, got in outs.items():
        bad = got != dered
        assert got.dtype == np.float32 and not bad.any(), \
            f"{lay}: {int(bad.sum())} of {got.size} samples differ, first at {np.argwhere(bad)[:1].tolist()}"
    per = run(monkeypatch, case, "aligned", xs, env=ENV[:1], normalise=False)
    assert np.array_equal(per.view(np.uint32), outs["aligned"].view(np.uint32)), "per-sample interpolation"
    assert np.array_equal(per, dered)


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_normalised_within_bound(rt, oracle, monkeypatch, name):
    case = CASES[name]
    xs, _, both, alone = refs(oracle, case)
    outs = {lay: run(monkeypatch, case, lay, xs) for lay in dc.LAYOUTS}
    outs["unfused"] = run(monkeypatch, case, "aligned", xs, env=ENV[1:2])
    outs["scalar"] = run(monkeypatch, case, "aligned", xs, env=ENV[1:])
    outs["per_sample"] = run(monkeypatch, case, "aligned", xs, env=ENV[:1])
    assert_variants(outs, both)
    # normalisation alone, in every layout and with scalar loads
    outs = {lay: run(monkeypatch, case, lay, xs, deredden=False) for lay in dc.LAYOUTS}
    outs["scalar"] = run(monkeypatch, case, "aligned", xs, env=ENV[2:], deredden=False)
    assert_variants(outs, alone)


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_interpolated_median_equals_oracle(rt, oracle, name):
    """rt.fast_running_median: the scrunch, the running median of the
    scrunched series and np.interp on their own (float64, float32 at scrunch
    factor 1), without the subtraction's rounding to float32."""
    case = CASES[name]
    for x in dc.series(case)[:2]:
        got = rt.fast_running_median(x, case["ws"], case["mp"])
        ref = oracle.fast_running_median(x, case["ws"], case["mp"])
        assert got.dtype == ref.dtype and np.array_equal(got, ref), int((got != ref).sum())


def test_neither_stage_copies(rt, oracle, monkeypatch):
    case = CASES["f5_mod2"]
    xs = dc.series(case)
    for lay in dc.LAYOUTS:
        assert np.array_equal(run(monkeypatch, case, lay, xs, deredden=False, normalise=False), xs)


RMED_KINDS = ("ties", "step", "inf")


def rmed_series(n, kind, seed):
    rs = np.random.RandomState(seed)
    if kind == "ties":
        x = np.round(rs.normal(size=n) * 2.0) / 2.0               # about a dozen distinct values
    elif kind == "step":
        x = np.where(np.arange(n) < n // 2, 100.0, -100.0) + rs.normal(size=n)
    else:
        u = rs.rand(n)
        x = np.where(u < 0.01, np.inf, np.where(u < 0.02, -np.inf, rs.normal(size=n)))
    return x.astype(np.float32)


@pytest.mark.parametrize("kind", RMED_KINDS)
@pytest.mark.parametrize("w,n", [(257, 258), (257, 1000), (257, 5003), (301, 302), (301, 1000), (301, 5003),
                                 (999, 1000), (999, 5003)])
def test_running_median_large_windows(rt, oracle, w, n, kind):
    """rmed_large_kernel (radix select, windows above 255) returns the value
    the reference's quickselect does: data with few distinct values, a step,
    and +-inf at 2 %, at n = w + 1 (every window clipped at both ends) and
    longer.  By value: the reference does not define which zero it returns."""
    x = rmed_series(n, kind, 1000 * w + n)
    got = rt.running_median(x, w)
    ref = oracle.running_median(x, w)
    assert got.dtype == np.float32 and np.array_equal(got, ref), int((got != ref).sum())
