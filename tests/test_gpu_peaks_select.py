"""The default peak selection on the GPU: rt_threshold_select_device
(threshold_select_kernel) against the selection restated in numpy
(peaks_select_common.ref_select), exact in counts and rows, at the shapes,
values and coefficient tables where the kernel can go wrong; then PeakFinder's
four ways to the peaks of riptide's find_peaks on synthetic S/N.

The kernel leaves a list's rows in no order, so a complete list is compared
sorted; of a truncated one the test asks what the caller relies on: the full
count, cap distinct members of the reference set, nothing written past them.
"""
import functools

import numpy as np
import pytest

import peaks_select_common as pc
import test_peaks_cluster_host as ph
from test_peaks_cluster_host import CANARY_ROW, SMIN

pytestmark = pytest.mark.gpu

COUNT_GARBAGE = 0x5A5A5A5A      # what the counts hold before the call: the entry point resets them
TAIL = 8                        # canary slots after either output


@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from riptide_amd import _lib
    return _lib.load()


def output_buffers(nlists, cap):
    """(counts, idx) on the device: nlists garbage counts and nlists * cap
    canary rows, TAIL more of each after the end."""
    import torch
    counts = torch.full((nlists + TAIL,), COUNT_GARBAGE, dtype=torch.int32, device="cuda")
    idx = torch.from_numpy(np.full(nlists * cap + TAIL, CANARY_ROW, dtype=np.uint32).view(np.int32)).cuda()
    return counts, idx


def read_back(counts, idx):
    import torch
    torch.cuda.synchronize()
    return counts.cpu().numpy().astype(np.int64), idx.cpu().numpy().view(np.uint32)


def device_select(lib, snrs, logf, coeffs, smin, cap, pad=5):
    """rt_threshold_select_device on snrs [B, L, W] uploaded at a stride of
    L * W + pad floats (the padding 1e9: a stray read would be selected), the
    counts prefilled with garbage and the lists with canaries: (counts
    [B, W], idx [B, W, cap]); asserts the slots after either array's end."""
    import torch
    from riptide_amd import _lib
    snrs = np.ascontiguousarray(snrs, dtype=np.float32)
    B, L, W = snrs.shape
    stride = L * W + pad
    host = np.full((B, stride), np.float32(1e9))
    host[:, :L * W] = snrs.reshape(B, -1)
    d_snrs = torch.from_numpy(host).cuda()
    coeffs = np.array(coeffs, dtype=np.float64)
    assert coeffs.shape[:2] == (B, W)
    d_logf = torch.from_numpy(np.array(logf, dtype=np.float64)).cuda()
    d_coeffs = torch.from_numpy(coeffs).cuda()
    counts, idx = output_buffers(B * W, cap)
    rc = lib.rt_threshold_select_device(_lib.ptr(d_snrs), B, stride, L, W, _lib.ptr(d_logf), _lib.ptr(d_coeffs),
                                        coeffs.shape[-1], smin, _lib.ptr(counts), _lib.ptr(idx), cap, None)
    assert rc == 0, lib.rt_last_error()
    counts, idx = read_back(counts, idx)
    assert (counts[B * W:] == COUNT_GARBAGE).all(), "counts written past the batch"
    assert (idx[B * W * cap:] == CANARY_ROW).all(), "rows written past the last list"
    return counts[:B * W].reshape(B, W), idx[:B * W * cap].reshape(B, W, cap)


def select_refs(snrs, logf, coeffs, smin):
    """ref_select of every (trial, width): [B][W] row arrays."""
    B, _, W = snrs.shape
    return [[pc.ref_select(snrs[b, :, iw], logf, coeffs[b, iw], smin) for iw in range(W)] for b in range(B)]


def assert_select(lib, snrs, logf, coeffs, smin, cap, refs=None):
    """Every (trial, width) against the restatement: the count in full; a
    complete list sorted equals the reference rows, a truncated one holds cap
    distinct reference rows; every slot from min(count, cap) on still holds
    the canary (the neighbouring lists' slots are checked as theirs, the tail
    by device_select).  Returns the reference counts [B, W]."""
    snrs = np.asarray(snrs, dtype=np.float32)
    coeffs = np.asarray(coeffs, dtype=np.float64)
    refs = refs if refs is not None else select_refs(snrs, logf, coeffs, smin)
    counts, idx = device_select(lib, snrs, logf, coeffs, smin, cap)
    for b, trial in enumerate(refs):
        for iw, ref in enumerate(trial):
            assert counts[b, iw] == len(ref), (b, iw, counts[b, iw], len(ref))
            k = min(len(ref), cap)
            got = idx[b, iw, :k].astype(np.int64)
            if len(ref) <= cap:
                assert np.array_equal(np.sort(got), ref), (b, iw)
            else:
                assert len(np.unique(got)) == cap and np.isin(got, ref).all(), (b, iw, got)
            assert (idx[b, iw, k:] == CANARY_ROW).all(), (b, iw)
    return np.array([[len(r) for r in trial] for trial in refs])


# --------------------------------------------------------------------------
# shapes: L around the 256-thread block, one to 37 widths (the row stride and
# the grid's second axis), one and two trials, caps at, below and far below
# the counts
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_case(length, widths, ncoef):
    """(snrs [2, L, W], logf, coeffs [2, W, ncoef]) from the clustering tests'
    random columns (random_case: noise with bumps well above the threshold):
    the first `length` rows of the 257- or 3000-row cases, their three
    columns as they are and, for more widths, rolled copies; every trial and
    width with coefficients of its own."""
    base = 3000 if length > 257 else 257
    cases = [ph.random_case(base, seed, ncoef) for seed in ph.SEEDS[base]]
    logf = cases[0][1][:length]
    copies = (widths + 2) // 3
    rolls = [0] + list(np.random.RandomState(100 * length + widths).randint(0, base, size=copies - 1))
    snrs = np.stack([np.concatenate([np.roll(c[0], k, axis=0) for k in rolls], axis=1)[:length, :widths]
                     for c in cases])
    coeffs = np.stack([np.concatenate([c[3] * (1.0 + 0.01 * b + 0.003 * k) for k in range(copies)])[:widths]
                       for b, c in enumerate(cases)])
    if length == 1:     # a lone row: selected in every other column
        snrs[:, 0, ::2] = 9.0
    for a in (snrs, coeffs):
        a.setflags(write=False)
    return snrs, logf, coeffs


@pytest.mark.parametrize("widths", [1, 3, 37])
@pytest.mark.parametrize("length", [1, 255, 256, 257, 3000])
def test_select_matches_numpy(lib, length, widths):
    """Counts and rows of every (trial, width) against ref_select, with a
    constant and a parabolic threshold, one and two trials, and cap = L (every
    list complete), 4 and 1 (most lists truncated)."""
    seen = []
    for ncoef in (1, 3):
        snrs, logf, coeffs = shape_case(length, widths, ncoef)
        if widths == 3 and length in ph.SEEDS:      # the random columns themselves: their own honesty condition
            for b, seed in enumerate(ph.SEEDS[length]):
                _, _, freqs, _, r = ph.random_case(length, seed, ncoef)
                assert ph.honest_enough(ph.ref_trial(snrs[b], logf, freqs, coeffs[b], SMIN, r)), (length, b)
        for batch in (1, 2):
            refs = select_refs(snrs[:batch], logf, coeffs[:batch], SMIN)
            for cap in (length, 4, 1):
                seen.append(assert_select(lib, snrs[:batch], logf, coeffs[:batch], SMIN, cap, refs))
    # on the restatement alone: selected rows in every launch, and from 255 rows on lists beyond cap = 4
    # (truncated there, complete at cap = length) of different lengths
    assert all(c.max() >= 1 for c in seen)
    if length >= 255:
        assert all(c.max() > 4 for c in seen)
        if widths > 1:
            assert all(len(np.unique(c)) > 1 for c in seen)


def test_all_and_none_selected(lib):
    """A column with every row selected beside one with none, swapped in the
    second trial: the count L, a truncated list of cap rows, and a list
    nothing is written to."""
    length = 600
    freqs, _ = ph.plan_grid(length)
    logf = np.log(freqs)
    s = np.zeros((2, length, 3), dtype=np.float32)
    s[0, :, 0] = s[0, :, 2] = s[1, :, 1] = 9.0
    coeffs = np.full((2, 3, 1), SMIN)
    for cap in (length, 4):
        want = assert_select(lib, s, logf, coeffs, SMIN, cap)
        assert want.tolist() == [[length, 0, length], [0, length, 0]]


# --------------------------------------------------------------------------
# values: equal to the bound, rounding-sensitive, not finite, signed zeros
# --------------------------------------------------------------------------
def rows_of(refs):
    return [[r.tolist() for r in trial] for trial in refs]


def test_threshold_equality(lib):
    """S/N equal to the constant threshold or to smin is not selected; the
    float32 one ulp above is."""
    pc.check_equality_cases()
    logf, _ = ph.synthetic(pc.EQ_LENGTH)
    for name, s, coeffs, smin, want in pc.equality_cases():
        refs = select_refs(s[None], logf, coeffs[None], smin)
        assert rows_of(refs) == [want], name
        for cap in (pc.EQ_LENGTH, 1):
            assert_select(lib, s[None], logf, coeffs[None], smin, cap, refs)


@pytest.mark.parametrize("degree", sorted(pc.RND_EACH))
def test_threshold_rounding(lib, degree):
    """Polynomials whose fused evaluation would change the comparison:
    np.polyval's two roundings per step decide, in both directions."""
    pc.check_rounding_cases()
    snrs, logf, _, coeffs, smin, _, want = pc.rounding_batch(degree)
    refs = select_refs(snrs, logf, coeffs, smin)
    assert rows_of(refs) == want
    assert_select(lib, snrs, logf, coeffs, smin, 4, refs)
    # the same cases behind a leading +0.0 coefficient, as poly1d_table would store them
    padded = np.concatenate([np.zeros(coeffs.shape[:2] + (1,)), coeffs], axis=-1)
    assert rows_of(select_refs(snrs, logf, padded, smin)) == want
    assert_select(lib, snrs, logf, padded, smin, 4, refs)


def test_not_finite_and_signed_zero(lib):
    """NaN and -inf are never selected, +inf always is (the bounds are
    finite); -0.0 equals +0.0 on either side of the comparison, and the
    smallest float32 denormal is above both."""
    length = 300
    freqs, _ = ph.plan_grid(length)
    logf = np.log(freqs)
    tiny = np.float32(1e-45)
    assert tiny > 0 and float(tiny) == 2.0 ** -149
    s = np.zeros((2, length, 4), dtype=np.float32)
    # trial 0: the values that are not finite, mixed in column 0, alone in the others
    for i, v in {3: np.nan, 64: np.inf, 65: -np.inf, 100: 3.0e38, 255: np.nan, 256: np.inf, 257: -3.0e38,
                 299: np.inf}.items():
        s[0, i, 0] = v
    s[0, :, 1] = np.nan
    s[0, :, 2] = -np.inf
    s[0, :, 3] = np.inf
    # trial 1: zeros of either sign and the denormals around them
    for i, v in {0: -0.0, 1: 0.0, 2: tiny, 3: -tiny, 255: tiny, 256: -0.0, 257: 0.0, 299: tiny}.items():
        s[1, i, 0] = v
    s[1, :, 1] = 0.0
    s[1, :, 2] = -0.0
    s[1, :, 3] = tiny
    assert np.signbit(s[1, 0, 0]) and np.signbit(s[1, :, 2]).all() and not np.signbit(s[1, :, 1]).any()
    # trial 0 against the constant 6; trial 1 under a polynomial below zero, so that smin decides
    coeffs = np.zeros((2, 4, 2))
    coeffs[0, :, 1] = SMIN
    coeffs[1, :, 1] = -1.0
    every = list(range(length))
    refs = select_refs(s, logf, coeffs, SMIN)
    assert rows_of(refs) == [[[64, 100, 256, 299], [], [], every], [[], [], [], []]]
    assert_select(lib, s, logf, coeffs, SMIN, length, refs)
    for smin in (0.0, -0.0):
        refs = select_refs(s, logf, coeffs, smin)
        assert rows_of(refs) == [[[64, 100, 256, 299], [], [], every], [[2, 255, 299], [], [], every]], smin
        assert_select(lib, s, logf, coeffs, smin, length, refs)
    # the zero polynomial of either sign above smin: s > 0.0 decides
    for zero in (0.0, -0.0):
        table = np.full((2, 4, 1), zero)
        assert rows_of(select_refs(s, logf, table, -1.0)) == rows_of(refs)
        assert_select(lib, s, logf, table, -1.0, length, refs)


# --------------------------------------------------------------------------
# coefficient tables
# --------------------------------------------------------------------------
def test_coefficient_tables(lib):
    """Leading +0.0 coefficients as poly1d_table stores a trimmed fit
    ([0, 0, a, b] selects what [a, b] selects; three zeros select what smin
    alone does) and the longest table the entry point takes: 61 zeros, then
    a parabola."""
    cases = [ph.random_case(257, seed, 3) for seed in ph.SEEDS[257]]
    logf = cases[0][1]
    snrs = np.stack([c[0] for c in cases])
    # the random cases' gentle parabolas lifted from 6.5 to 9.5 and lines through 11 + b at the grid's middle:
    # both inside the bumps' heights, so neither selects what the other or smin alone does
    parabolas = np.stack([c[3] * (1.0 + 0.01 * b) + [0.0, 0.0, 3.0] for b, c in enumerate(cases)])
    slopes = 1.5 + np.arange(3.0)
    lines = np.stack([np.stack([slopes, 11.0 + b - slopes * logf.mean()], axis=1) for b in range(2)])
    plain = select_refs(snrs, logf, parabolas, SMIN)
    seen = {}
    for name, (table, same_as) in pc.coefficient_tables(parabolas, lines).items():
        refs = select_refs(snrs, logf, table, SMIN)
        assert rows_of(refs) == rows_of(select_refs(snrs, logf, same_as, SMIN)), name
        for cap in (257, 4):
            counts = assert_select(lib, snrs, logf, table, SMIN, cap, refs)
        assert counts.max() > 4, name
        assert_select(lib, snrs, logf, same_as, SMIN, 257, refs)
        seen[name] = rows_of(refs)
    # the three kinds of table select differently: the coefficients are read, whatever their number
    assert seen["[0, a, b]"] == seen["[0, 0, a, b]"] and seen["61 zeros, parabola"] == rows_of(plain)
    assert seen["[0, a, b]"] != seen["zero polynomial"] != seen["61 zeros, parabola"] != seen["[0, a, b]"]


# --------------------------------------------------------------------------
# empty shapes and refusals
# --------------------------------------------------------------------------
def test_empty_shapes(lib):
    """length 0 zeroes the counts and writes no row; a batch or a width
    count of 0 touches nothing."""
    import torch
    from riptide_amd import _lib
    counts, idx = device_select(lib, np.zeros((2, 0, 3), dtype=np.float32), np.zeros(0), np.full((2, 3, 1), SMIN),
                                SMIN, cap=4)
    assert counts.tolist() == [[0, 0, 0], [0, 0, 0]] and (idx == CANARY_ROW).all()
    d_snrs = torch.full((64,), 1e9, dtype=torch.float32, device="cuda")
    d_logf = torch.zeros(8, dtype=torch.float64, device="cuda")
    d_coeffs = torch.zeros(8, dtype=torch.float64, device="cuda")
    for batch, widths in ((0, 3), (2, 0), (0, 0)):
        counts, idx = output_buffers(6, 4)
        rc = lib.rt_threshold_select_device(_lib.ptr(d_snrs), batch, 24, 8, widths, _lib.ptr(d_logf),
                                            _lib.ptr(d_coeffs), 1, SMIN, _lib.ptr(counts), _lib.ptr(idx), 4, None)
        assert rc == _lib.RT_OK, lib.rt_last_error()
        counts, idx = read_back(counts, idx)
        assert (counts == COUNT_GARBAGE).all() and (idx == CANARY_ROW).all(), (batch, widths)


def test_refusals(lib):
    """ncoef 0 and 65 and a batch of 65536 are refused with the entry point's
    message before anything is launched: the outputs keep their canaries."""
    import torch
    from riptide_amd import _lib
    d_snrs = torch.full((2 * 8 * 3,), 9.0, dtype=torch.float32, device="cuda")      # every row would be selected
    d_logf = torch.zeros(8, dtype=torch.float64, device="cuda")
    d_coeffs = torch.zeros(2 * 3 * 65, dtype=torch.float64, device="cuda")
    for kw, text in ((dict(ncoef=0), b"1 to 64 polynomial coefficients"),
                     (dict(ncoef=65), b"1 to 64 polynomial coefficients"),
                     (dict(batch=65536), b"threshold selection too large")):
        a = dict(batch=2, ncoef=1)
        a.update(kw)
        counts, idx = output_buffers(6, 4)
        rc = lib.rt_threshold_select_device(_lib.ptr(d_snrs), a["batch"], 24, 8, 3, _lib.ptr(d_logf),
                                            _lib.ptr(d_coeffs), a["ncoef"], SMIN, _lib.ptr(counts), _lib.ptr(idx), 4,
                                            None)
        assert rc == _lib.RT_EINVAL, kw
        assert text in lib.rt_last_error(), (kw, lib.rt_last_error())
        counts, idx = read_back(counts, idx)
        assert (counts == COUNT_GARBAGE).all() and (idx == CANARY_ROW).all(), kw
    # the same buffers, accepted: the refusals above were not for want of a valid call
    counts, idx = output_buffers(6, 4)
    rc = lib.rt_threshold_select_device(_lib.ptr(d_snrs), 2, 24, 8, 3, _lib.ptr(d_logf), _lib.ptr(d_coeffs), 64,
                                        SMIN, _lib.ptr(counts), _lib.ptr(idx), 4, None)
    assert rc == _lib.RT_OK, lib.rt_last_error()
    counts, idx = read_back(counts, idx)
    assert counts[:6].tolist() == [8] * 6 and (counts[6:] == COUNT_GARBAGE).all()
    assert (idx[:24] < 8).all() and (idx[24:] == CANARY_ROW).all()


# --------------------------------------------------------------------------
# PeakFinder: four ways to find_peaks' peaks
# --------------------------------------------------------------------------
FINDER_PATHS = {
    "default": {},
    "default, truncated lists": {"max_selected": pc.FINDER_MAX_SELECTED},
    "device_cluster": {"device_cluster": True},
    "device_cluster, max_peaks=1": {"device_cluster": True, "max_peaks": 1},
}


@pytest.fixture(scope="module")
def finder_inputs():
    """The small search's plan and finder_case()'s S/N on the device."""
    import torch
    from riptide_amd import engine
    c = pc.FINDER_SEARCH
    widths, periods, foldbins, tobs, snrs = pc.finder_case()
    plan = engine.PeriodogramPlan.for_search(c["n"], c["tsamp"], c["pmin"], c["pmax"], c["bmin"], c["bmax"],
                                             ducy_max=c["ducy_max"])
    p, fb = plan.grid()
    assert np.array_equal(p, periods) and np.array_equal(fb, foldbins), "the plan's grid is the host planner's"
    assert np.array_equal(plan.widths, widths)
    return plan, tobs, torch.from_numpy(np.array(snrs)).cuda()


@pytest.mark.parametrize("branch", sorted(pc.FINDER_BRANCHES))
def test_peak_finder_four_ways(finder_inputs, branch):
    """The default path, the default path with lists truncated at 4 rows
    (the host mask beside gathered lists), device clustering, and device
    clustering truncated at one cluster each return exactly find_peaks of
    the same array: identical Peak tuples in order, identical polycos; in
    the polynomial branch and in the constant-threshold one."""
    from riptide_amd.peaks import PeakFinder
    pc.check_finder_case()
    plan, tobs, snr = finder_inputs
    ref = pc.finder_reference(branch)
    for name, kw in FINDER_PATHS.items():
        got = PeakFinder(plan, tobs, **kw, **pc.FINDER_BRANCHES[branch])(snr, dms=list(pc.FINDER_DMS))
        assert len(got) == len(ref) == 2
        for b in range(2):
            assert got[b][0] == ref[b][0], (name, b)
            assert sorted(got[b][1]) == sorted(ref[b][1]), (name, b)
            for iw in ref[b][1]:
                assert np.array_equal(np.asarray(got[b][1][iw]), np.asarray(ref[b][1][iw])), (name, b, iw)
