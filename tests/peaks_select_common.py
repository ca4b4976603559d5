"""Inputs that pin the threshold selection (s > polyval(coef, log f)) & (s >
smin) to numpy where an implementation can differ from it without any
periodogram noticing: S/N equal to the threshold or to smin, polynomials for
which a fused multiply-add changes the comparison, coefficient tables in
poly1d_table's form, and the synthetic S/N arrays PeakFinder's paths are
compared on.  Everything here is host numpy, seeded, and checked against the
restatement alone (the check_* functions, run by
tests/test_peaks_cluster_host.py without a GPU).

Shared by tests/test_gpu_peaks_select.py (rt_threshold_select_device,
PeakFinder), tests/test_peaks_cluster_host.py (rt_find_peaks_host) and
tests/test_gpu_peaks_cluster.py (rt_find_peaks_device).
"""
import ctypes
import functools
from fractions import Fraction

import numpy as np

from test_peaks_cluster_host import SMIN, plan_grid, random_case, ref_column, synthetic  # noqa: F401

F32 = np.float32


def ref_select(col, logf, coef, smin):
    """The selection restated: the rows np.where leaves, ascending."""
    with np.errstate(invalid="ignore"):
        return np.where((col.astype(float) > np.poly1d(coef)(logf)) & (col.astype(float) > smin))[0]


def ulps(v, k):
    """The float32 k ulps above (k > 0) or below (k < 0) float32 v."""
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf), dtype=F32)
    return v


# --------------------------------------------------------------------------
# S/N equal to the threshold, equal to smin
# --------------------------------------------------------------------------
EQ_LENGTH = 70
# the values sat on: an ordinary one, one whose lower neighbour is half an ulp
# away (a power of two), a small one, a negative one
EQ_VALUES = tuple(F32(v) for v in (7.3, 8.0, 6.0000005, -3.25))


def _triplet(col, i, v):
    """v - 1 ulp, v, v + 1 ulp in rows i, i + 1, i + 2; the selected row."""
    col[i:i + 3] = (ulps(v, -1), v, ulps(v, +1))
    return i + 2


@functools.lru_cache(maxsize=None)
def equality_cases():
    """[(name, snrs [L, W] float32, coeffs [W, 1], smin, expected rows per
    column)] on the grid of synthetic(EQ_LENGTH): constant thresholds that are
    exactly a float32 S/N of the column (the polynomial, smin, or both), with
    the values one float32 ulp below and above in the neighbouring rows.
    Only the row one ulp above is selected; a radius below the grid's step
    (0.25) keeps every selected row a cluster of its own, so a row selected
    by `>=` shows as a peak too."""
    W = len(EQ_VALUES)
    cases = []
    # the polynomial sits on the value, smin is far below
    s = np.full((EQ_LENGTH, W), F32(-50.0))
    want = [[_triplet(s[:, iw], 10 + 7 * iw, v)] for iw, v in enumerate(EQ_VALUES)]
    cases.append(("threshold", s, np.array([[float(v)] for v in EQ_VALUES]), -40.0, want))
    # smin sits on the value, the polynomial is far below
    for v in EQ_VALUES:
        s = np.full((EQ_LENGTH, W), F32(-50.0))
        want = [[_triplet(s[:, iw], 3 + 20 * iw, v)] for iw in range(W)]
        cases.append((f"smin={v}", s, np.full((W, 1), -40.0), float(v), want))
    # both sit on values of the column: the higher one decides, whichever it is
    lo, hi = EQ_VALUES[0], EQ_VALUES[1]
    s = np.full((EQ_LENGTH, 2), F32(-50.0))
    want = []
    for iw in range(2):
        _triplet(s[:, iw], 5, lo)          # all three above the lower bound, none above the higher
        want.append([_triplet(s[:, iw], 40, hi)])
    want[0].insert(0, 0)
    s[0, 0] = np.inf
    cases.append(("both, smin higher", s, np.full((2, 1), float(lo)), float(hi), want))
    cases.append(("both, threshold higher", s, np.full((2, 1), float(hi)), float(lo), want))
    for _, s, c, _, _ in cases:
        s.setflags(write=False)
        c.setflags(write=False)
    return cases


def check_equality_cases():
    """The precondition, on the restatement alone: every case has a row equal
    to its bound, and numpy selects exactly the rows one ulp above."""
    logf, _ = synthetic(EQ_LENGTH)
    for name, s, coeffs, smin, want in equality_cases():
        for iw in range(s.shape[1]):
            col = s[:, iw].astype(float)
            assert (col == coeffs[iw, 0]).any() or (col == smin).any(), name
            assert ref_select(s[:, iw], logf, coeffs[iw], smin).tolist() == want[iw], (name, iw)
            # `>=` would add the row below each expected one
            with_equal = np.where((col >= coeffs[iw, 0]) & (col >= smin))[0]
            assert len(with_equal) > len(want[iw]), (name, iw)


# --------------------------------------------------------------------------
# polynomials for which a fused multiply-add changes the comparison
# --------------------------------------------------------------------------
RND_LENGTH = 600
RND_SEED = 20240607
RND_EACH = {1: 8, 2: 4}         # cases per direction, by degree


def _fused(a, x, c):
    """fl(a * x + c): one rounding (Fraction.__float__ is a correctly rounded
    integer division)."""
    return float(Fraction(a) * Fraction(x) + Fraction(c))


def horner_fused(coef, x):
    """np.polyval's loop with every y * x + c a fused multiply-add."""
    y = 0.0
    for c in coef:
        y = _fused(y, x, float(c))
    return y


def _nudge(v, k):
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return float(v)


@functools.lru_cache(maxsize=None)
def rounding_cases(degree):
    """(numpy_selects, fused_selects): two lists of RND_EACH[degree] cases
    (row i, coefficients highest degree first, float32 s) on the grid
    plan_grid(RND_LENGTH), found by a seeded search: s > np.polyval(coef,
    logf[i]) differs from s > horner_fused(coef, logf[i]).  In the first list
    numpy's two roundings per step select the row and a fused evaluation
    rejects it; in the second the reverse.

    The draws: a random row, leading coefficients drawn freely, s in
    (6.5, 7.9), and the constant term the double nearest s - (the rest),
    nudged by -3..3 ulps, so that the polynomial lands within a few ulps of
    s and the last step's rounding decides."""
    rng = np.random.RandomState(RND_SEED + degree)
    freqs, _ = plan_grid(RND_LENGTH)
    logf = np.log(freqs)
    need = RND_EACH[degree]
    found = ([], [])
    rows = set()
    for _ in range(20000):
        i = int(rng.randint(0, RND_LENGTH))
        x = float(logf[i])
        s = F32(rng.uniform(6.5, 7.9))
        if degree == 1:
            lead = [rng.uniform(2.0, 8.0)]
        else:
            lead = [rng.uniform(0.05, 0.5), rng.uniform(-2.0, 2.0)]
        partial = float(np.polyval(lead, x)) * x
        coef = lead + [_nudge(float(s) - partial, int(rng.randint(-3, 4)))]
        y2, yf = float(np.polyval(coef, x)), horner_fused(coef, x)
        if (float(s) > y2) == (float(s) > yf) or i in rows:
            continue
        which = found[0] if float(s) > y2 else found[1]
        if len(which) < need:
            which.append((i, tuple(coef), s))
            rows.add(i)
        if len(found[0]) == need and len(found[1]) == need:
            break
    return found


def rounding_batch(degree):
    """The rounding cases as a batch of two trials: (snrs [2, L, W] float32,
    logf, freqs, coeffs [2, W, degree + 1], smin, radius, expected rows [2][W]).
    Trial 0 holds the cases numpy selects, trial 1 those only a fused
    evaluation would; each case is alone in its column, at its own row, and
    smin = 6 keeps every other row (S/N 0) quiet wherever the polynomial
    goes."""
    sel, rej = rounding_cases(degree)
    W = RND_EACH[degree]
    freqs, tobs = plan_grid(RND_LENGTH)
    snrs = np.zeros((2, RND_LENGTH, W), dtype=F32)
    coeffs = np.zeros((2, W, degree + 1))
    want = [[], []]
    for b, cases in enumerate((sel, rej)):
        for iw, (i, coef, s) in enumerate(cases):
            snrs[b, i, iw] = s
            coeffs[b, iw] = coef
            want[b].append([i] if b == 0 else [])
    return snrs, np.log(freqs), freqs, coeffs, SMIN, 0.1 / tobs, want


def check_rounding_cases():
    """The precondition, on the restatement alone: enough cases of each
    direction, and each still discriminates under the vectorised evaluation
    ref_select uses (np.poly1d over the whole grid), which must be np.polyval's
    two roundings and not the fused value."""
    for degree, need in RND_EACH.items():
        sel, rej = rounding_cases(degree)
        assert len(sel) == need and len(rej) == need, (degree, len(sel), len(rej))
        snrs, logf, _, coeffs, smin, _, want = rounding_batch(degree)
        for b, cases in enumerate((sel, rej)):
            for iw, (i, coef, s) in enumerate(cases):
                y2 = float(np.poly1d(coef)(logf)[i])
                yf = horner_fused(coef, float(logf[i]))
                assert y2 == float(np.polyval(coef, logf[i])), (degree, b, iw)
                assert (float(s) > y2) == (b == 0) and (float(s) > yf) == (b == 1), (degree, b, iw, y2, yf, s)
                assert float(s) > smin
                assert ref_select(snrs[b, :, iw], logf, coeffs[b, iw], smin).tolist() == want[b][iw]


# --------------------------------------------------------------------------
# coefficient tables
# --------------------------------------------------------------------------
def coefficient_tables(parabolas, lines):
    """{name: (table [..., ncoef], the shorter table whose selection it must
    equal)} from a [..., 3] table of parabolas and a [..., 2] table of lines:
    leading +0.0 as poly1d_table stores trimmed fits (ncoef 3 and 4 around a
    line, ncoef 1: the zero polynomial), and ncoef 64: 61 zeros, then the
    parabola."""
    parabolas = np.asarray(parabolas, dtype=np.float64)
    lines = np.asarray(lines, dtype=np.float64)
    assert parabolas.shape[-1] == 3 and lines.shape[-1] == 2
    zeros = np.zeros(parabolas.shape[:-1] + (1,))

    def lead(n, tail):
        return np.concatenate([zeros] * n + [tail], axis=-1)

    return {
        "zero polynomial": (lead(2, zeros), zeros.copy()),
        "[0, a, b]": (lead(1, lines), lines),
        "[0, 0, a, b]": (lead(2, lines), lines),
        "61 zeros, parabola": (lead(61, parabolas), parabolas),
    }


# --------------------------------------------------------------------------
# PeakFinder's paths: synthetic S/N on a small search's grid
# --------------------------------------------------------------------------
FINDER_SEARCH = dict(n=1 << 16, tsamp=256e-6, pmin=0.1, pmax=1.0, bmin=240, bmax=260, ducy_max=0.2)
FINDER_SEED = 7
FINDER_DMS = (0.0, 5.0)
FINDER_MAX_SELECTED = 4
FINDER_RUN = 200               # the long run: at least this many selected rows in one column
FINDER_BRANCHES = {"polynomial": {}, "constant": {"minseg": 10 ** 6}}


@functools.lru_cache(maxsize=None)
def finder_case():
    """(widths, periods, foldbins, tobs, snrs [2, L, W] float32) on the grid
    of the small search (2^16 samples of 256 us, periods 0.1-1 s, 240-260
    bins: about 30 segments of 5 / tobs): noise N(0, 1) in trial 0 and
    N(0, 1.3^2) in trial 1, so the fitted thresholds differ; column 0 of
    either trial stays noise, column 1 gets one bump of 1-4 rows, the other
    columns bumps of 1-40 rows of height 8-14 at seeded places, and one
    column per trial a run of 220 rows at 30 (under a quarter of a segment's
    rows, so the segment's quartiles stay in the noise and the fit below the
    run)."""
    from riptide_amd import _lib
    from riptide_amd.ffautils import generate_width_trials
    c = FINDER_SEARCH
    lib = _lib.load()
    args = (c["n"], c["tsamp"], c["pmin"], c["pmax"], c["bmin"], c["bmax"])
    length = ctypes.c_size_t()
    assert lib.rt_periodogram_length(*args, ctypes.byref(length)) == 0
    L = length.value
    periods = np.empty(L)
    foldbins = np.empty(L, dtype=np.uint32)
    assert lib.rt_periodogram_grid(*args, _lib.ptr(periods), _lib.ptr(foldbins)) == 0
    widths = generate_width_trials(c["bmin"], ducy_max=c["ducy_max"])
    W = len(widths)
    rng = np.random.RandomState(FINDER_SEED)
    snrs = np.stack([rng.normal(scale=sigma, size=(L, W)) for sigma in (1.0, 1.3)]).astype(F32)
    for b in range(2):
        i0 = rng.randint(0, L - 4)
        n = rng.randint(1, 5)
        snrs[b, i0:i0 + n, 1] += (10.0 + 4.0 * rng.rand(n)).astype(F32)
        for iw in range(2, W):
            for _ in range(rng.randint(1, 6)):
                n = rng.randint(1, 41)
                i0 = rng.randint(0, L)
                i1 = min(L, i0 + n)
                snrs[b, i0:i1, iw] += (8.0 + 6.0 * rng.rand(i1 - i0)).astype(F32)
        i0 = rng.randint(0, L - 220)
        snrs[b, i0:i0 + 220, W - 1 - b] += F32(30.0)
    for a in (periods, foldbins, snrs):
        a.setflags(write=False)
    return widths, periods, foldbins, c["n"] * c["tsamp"], snrs


@functools.lru_cache(maxsize=None)
def finder_reference(branch):
    """find_peaks of every trial of finder_case(): [(peaks, polycos)]."""
    from riptide_amd.metadata import Metadata
    from riptide_amd.peak_detection import find_peaks
    from riptide_amd.periodogram import Periodogram
    widths, periods, foldbins, tobs, snrs = finder_case()
    return [find_peaks(Periodogram(widths, periods, foldbins, snrs[b], metadata=Metadata({"tobs": tobs, "dm": dm})),
                       **FINDER_BRANCHES[branch])
            for b, dm in enumerate(FINDER_DMS)]


def finder_selected_counts(branch):
    """Rows find_peaks_single selects in every (trial, width) of
    finder_case(), from the reference's own polycos: [2, W]."""
    widths, periods, _, _, snrs = finder_case()
    logf = np.log(1.0 / periods)
    ref = finder_reference(branch)
    return np.array([[len(ref_select(snrs[b, :, iw], logf, ref[b][1][iw], SMIN)) for iw in range(len(widths))]
                     for b in range(2)])


def check_finder_case():
    """The conditions that make finder_case() exercise PeakFinder's
    bookkeeping, on the reference alone, in both threshold branches: with
    max_selected = 4 every trial holds a column over the cap (host mask), a
    column of 1-4 selected rows (device list), a column of none and a column
    of FINDER_RUN selected rows or more; some column holds several clusters
    (the truncated path at max_peaks = 1); the polynomial branch fits a
    parabola per column, and the trials' fits differ."""
    _, periods, _, tobs, _ = finder_case()
    nseg = int(np.ceil(abs(1.0 / periods[-1] - 1.0 / periods[0]) / (5.0 / tobs)))
    assert 10 <= nseg < 10 ** 6, nseg
    for branch in FINDER_BRANCHES:
        counts = finder_selected_counts(branch)
        for b in range(2):
            c = counts[b]
            assert (c > FINDER_MAX_SELECTED).any() and (c == 0).any(), (branch, b, c)
            assert ((c >= 1) & (c <= FINDER_MAX_SELECTED)).any(), (branch, b, c)
            assert c.max() >= FINDER_RUN, (branch, b, c)
            per_width = np.bincount([p.iw for p in finder_reference(branch)[b][0]])
            assert per_width.max() >= 2, (branch, b, per_width)
    ref = finder_reference("polynomial")
    assert all(len(np.atleast_1d(ref[b][1][iw])) == 3 for b in range(2) for iw in ref[b][1])
    assert not np.array_equal(np.asarray(ref[0][1][0]), np.asarray(ref[1][1][0]))
    assert list(finder_reference("constant")[0][1][0]) == [SMIN]
