"""Peak clustering on the host: rt_find_peaks_host (peaks_host.hpp's serial
walk compiled for the CPU) against a literal numpy restatement of the tail of
riptide's find_peaks_single (riptide/peak_detection.py:130-141: np.where,
cluster1d, argmax), exact in rows, S/N bits and counts.

cluster1d sorts a cluster's points by ascending frequency before the argmax,
so of several equal maxima the one of lowest frequency is the peak: the first
(lowest) row on a grid whose frequencies rise with the row, the last on a
periodogram's own grid, where they fall.  The entry point's records are in
ascending row order on either grid; the restatement's peaks are sorted by row
for the comparison.

The seeded inputs and the restatement are shared with
tests/test_gpu_peaks_cluster.py.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

SMIN = 6.0
L_MAIN, W_MAIN = 3000, 3
CANARY_ROW, CANARY_SNR = 0xDEADBEEF, np.float32(-7777.0)
# seeds of the random columns, chosen with the restatement alone so that
# honest_enough() holds (at least half of the columns with two or more
# clusters, a cluster across a 64-row chunk boundary)
SEEDS = {3000: (11, 12), 257: (21, 22)}


@pytest.fixture(scope="module")
def lib():
    from riptide_amd import _lib
    return _lib.load()


# --------------------------------------------------------------------------
# the reference's rule, restated
# --------------------------------------------------------------------------
def ref_cluster1d(x, r):
    """riptide/clustering.py:4-51, already_sorted=False."""
    if not len(x):
        return []
    indices = x.argsort()
    diff = np.diff(x[indices])
    ibreaks = np.where(abs(diff) > r)[0]
    if not len(ibreaks):
        return [indices]
    ibounds = np.concatenate(([0], ibreaks + 1, [len(x)]))
    return [indices[start:end] for start, end in zip(ibounds[:-1], ibounds[1:])]


def ref_column(col, logf, freqs, coef, smin, r):
    """find_peaks_single's tail for one column: (peak rows ascending, their
    float32 S/N, the clusters as row arrays)."""
    s = col.astype(float)
    dynthr = np.poly1d(coef)(logf) if len(coef) else np.zeros_like(logf)
    with np.errstate(invalid="ignore"):
        mask = (s > dynthr) & (s > smin)
    indices = np.where(mask)[0]
    fsel = freqs[indices]
    peaks, clusters = [], []
    for cl in ref_cluster1d(fsel, r):
        ix = indices[cl]
        peaks.append(int(ix[s[ix].argmax()]))
        clusters.append(np.sort(ix))
    order = np.argsort(peaks)
    peaks = np.asarray(peaks, dtype=np.int64)[order]
    return peaks, col[peaks], [clusters[k] for k in order]


def ref_trial(snrs, logf, freqs, coeffs, smin, r):
    return [ref_column(snrs[:, iw], logf, freqs, coeffs[iw], smin, r) for iw in range(snrs.shape[1])]


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_grid(length):
    """The first `length` trial frequencies of a real plan grid
    (rt_periodogram_grid: 2^18 samples of 256 us, periods 0.1-1 s, 240-260
    bins) and its observation time."""
    from riptide_amd import _lib
    lib = _lib.load()
    n, tsamp, args = 1 << 18, 256e-6, (0.1, 1.0, 240, 260)
    full = ctypes.c_size_t()
    assert lib.rt_periodogram_length(n, tsamp, *args, ctypes.byref(full)) == 0
    assert full.value >= length
    periods = np.empty(full.value)
    bins = np.empty(full.value, dtype=np.uint32)
    assert lib.rt_periodogram_grid(n, tsamp, *args, _lib.ptr(periods), _lib.ptr(bins)) == 0
    freqs = np.ascontiguousarray(1.0 / periods[:length])
    freqs.setflags(write=False)
    return freqs, n * tsamp


@functools.lru_cache(maxsize=None)
def random_case(length, seed, ncoef):
    """(snrs [L, W] float32, logf, freqs, coeffs [W, ncoef], radius): N(0, 1)
    noise with bumps of 1-40 rows well above the threshold, on the plan grid."""
    rng = np.random.RandomState(seed)
    freqs, tobs = plan_grid(length)
    logf = np.log(freqs)
    snrs = rng.normal(size=(length, W_MAIN)).astype(np.float32)
    for iw in range(W_MAIN):
        for _ in range(max(4, length // 120)):
            n = rng.randint(1, 41)
            i0 = rng.randint(0, length)
            i1 = min(length, i0 + n)
            snrs[i0:i1, iw] += (8.0 + 6.0 * rng.rand(i1 - i0)).astype(np.float32)
    if ncoef == 1:
        coeffs = np.full((W_MAIN, 1), SMIN)
    else:   # a gentle parabola in log f around 6.5
        mid = logf.mean()
        coeffs = np.array([[0.05 * (iw + 1), -0.1 * (iw + 1) * mid, 6.5 + 0.05 * (iw + 1) * mid * mid]
                           for iw in range(W_MAIN)])
    for a in (snrs, logf, coeffs):
        a.setflags(write=False)
    return snrs, logf, freqs, coeffs, 0.1 / tobs


def honest_enough(ref, chunk=64):
    """The condition that keeps the random cases honest, on the restatement's
    output: at least half of the columns hold two or more clusters and at
    least one cluster crosses a chunk boundary."""
    many = sum(len(rows) >= 2 for rows, _, _ in ref)
    crossing = any(cl[0] // chunk != cl[-1] // chunk for _, _, cls in ref for cl in cls)
    return 2 * many >= len(ref) and crossing


def host_find(lib, snrs, logf, freqs, coeffs, smin, r, cap, pad=8):
    """rt_find_peaks_host with canary words after every array: (counts, rows
    [W, cap], snr [W, cap]); asserts the canaries."""
    from riptide_amd import _lib
    snrs = np.ascontiguousarray(snrs, dtype=np.float32)
    L, W = snrs.shape
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    counts = np.full(W + pad, CANARY_ROW, dtype=np.uint32)
    rows = np.full(W * cap + pad, CANARY_ROW, dtype=np.uint32)
    out = np.full(W * cap + pad, CANARY_SNR, dtype=np.float32)
    rc = lib.rt_find_peaks_host(_lib.ptr(snrs), L, W, _lib.ptr(np.ascontiguousarray(logf)),
                                _lib.ptr(np.ascontiguousarray(freqs)), _lib.ptr(coeffs), coeffs.shape[1], smin, r,
                                _lib.ptr(counts), _lib.ptr(rows), _lib.ptr(out), cap)
    assert rc == 0, lib.rt_last_error()
    assert (counts[W:] == CANARY_ROW).all() and (rows[W * cap:] == CANARY_ROW).all()
    assert (out[W * cap:] == CANARY_SNR).all()
    return counts[:W].astype(np.int64), rows[:W * cap].reshape(W, cap), out[:W * cap].reshape(W, cap)


def assert_matches(ref, counts, rows, out, cap):
    """Counts in full, the first min(count, cap) records exact (S/N by bits),
    nothing written past them."""
    for iw, (prow, psnr, _) in enumerate(ref):
        assert counts[iw] == len(prow), (iw, counts[iw], len(prow))
        k = min(len(prow), cap)
        assert np.array_equal(rows[iw, :k], prow[:k]), iw
        assert np.array_equal(out[iw, :k].view(np.uint32), psnr[:k].view(np.uint32)), iw
        assert (rows[iw, k:] == CANARY_ROW).all() and (out[iw, k:] == CANARY_SNR).all(), iw


def check(lib, snrs, logf, freqs, coeffs, r, cap, smin=SMIN):
    ref = ref_trial(snrs, logf, freqs, coeffs, smin, r)
    assert_matches(ref, *host_find(lib, snrs, logf, freqs, coeffs, smin, r, cap), cap)
    return ref


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
@pytest.mark.parametrize("ncoef", [1, 3])
@pytest.mark.parametrize("length", sorted(SEEDS))
def test_random_columns(lib, length, ncoef):
    for seed in SEEDS[length]:
        snrs, logf, freqs, coeffs, r = random_case(length, seed, ncoef)
        ref = check(lib, snrs, logf, freqs, coeffs, r, cap=length)
        assert honest_enough(ref), (length, seed, ncoef)


def synthetic(length, rising=True):
    freqs = np.arange(length) * 0.25 + 1.0
    if not rising:
        freqs = freqs[::-1].copy()
    return np.log(freqs), freqs


def column(length, spikes, width=1):
    s = np.zeros((length, width), dtype=np.float32)
    for i, v in spikes.items():
        s[i, 0] = v
    return s


def test_gap_equal_to_radius_does_not_split(lib):
    logf, freqs = synthetic(64)
    s = column(64, {3: 9.0, 4: 10.0, 5: 9.5, 7: 11.0, 8: 8.0, 20: 9.0})
    ref = check(lib, s, logf, freqs, [[SMIN]], 0.25, cap=64)
    assert list(ref[0][0]) == [4, 7, 20]             # 3-5 one cluster (gaps 0.25), 7-8 (gap 0.5 from 5), 20
    below = np.nextafter(0.25, 0.0)
    ref = check(lib, s, logf, freqs, [[SMIN]], below, cap=64)
    assert list(ref[0][0]) == [3, 4, 5, 7, 8, 20]    # one ulp less: every selected row alone


@pytest.mark.parametrize("rising", [True, False])
def test_ties_go_to_the_lowest_frequency(lib, rising):
    """Two and three equal maxima in one cluster: np.argmax over the cluster
    sorted by ascending frequency -- the lowest row on a rising grid, the
    highest on a falling one."""
    logf, freqs = synthetic(40, rising)
    s = column(40, {2: 9.0, 3: 12.0, 4: 12.0, 5: 7.0, 20: 8.0, 21: 15.0, 22: 9.0, 23: 15.0, 24: 15.0, 25: 7.0})
    ref = check(lib, s, logf, freqs, [[SMIN]], 0.25, cap=40)
    assert list(ref[0][0]) == ([3, 21] if rising else [4, 24])


def test_edges_and_specials(lib):
    logf, freqs = synthetic(50)
    one = [[SMIN]]
    # nothing selected
    ref = check(lib, column(50, {}), logf, freqs, one, 0.25, cap=4)
    assert len(ref[0][0]) == 0
    # every row selected: one cluster, and the ends of the column
    s = np.full((50, 1), 7.0, dtype=np.float32)
    s[49, 0] = 8.0
    ref = check(lib, s, logf, freqs, one, 0.25, cap=4)
    assert list(ref[0][0]) == [49]
    ref = check(lib, column(50, {0: 9.0, 49: 9.5}), logf, freqs, one, 0.25, cap=4)
    assert list(ref[0][0]) == [0, 49]
    # NaN is never selected and splits nothing by itself; +inf is a value
    s = column(50, {10: 9.0, 11: np.nan, 12: 9.5, 30: np.inf, 31: 1e30, 40: np.nan})
    ref = check(lib, s, logf, freqs, one, 0.5, cap=4)
    assert list(ref[0][0]) == [12, 30]
    # a threshold polynomial above smin, and smin above the polynomial
    ref = check(lib, column(50, {5: 9.0, 25: 11.0}), logf, freqs, [[0.0, 10.0]], 0.25, cap=4)
    assert list(ref[0][0]) == [25]
    ref = check(lib, column(50, {5: 9.0, 25: 11.0}), logf, freqs, [[1.0]], 0.25, cap=4, smin=10.0)
    assert list(ref[0][0]) == [25]


def test_cap_below_the_cluster_count(lib):
    """The count is reported in full, the first cap records are valid and
    nothing is written past them (host_find's canaries and assert_matches'),
    in this column and in its neighbour."""
    logf, freqs = synthetic(100)
    s = np.zeros((100, 2), dtype=np.float32)
    s[5:95:10, 0] = np.arange(9, dtype=np.float32) + 8.0      # 9 clusters
    s[[20, 60], 1] = 9.0                                      # 2 clusters
    ref = check(lib, s, logf, freqs, [[SMIN], [SMIN]], 0.25, cap=4)
    assert [len(r[0]) for r in ref] == [9, 2]


def test_threshold_equality_and_rounding(lib):
    """The walk's selection where `>=` for `>` or a fused y * x + c would
    show (peaks_select_common): an S/N equal to the constant threshold or to
    smin is not selected while the float32 one ulp above it is, and
    polynomials for which a fused multiply-add changes the comparison follow
    np.polyval's two roundings per step (the host's -ffp-contract=off), in
    both directions.  Every selected row is a cluster of its own, so the
    peaks are the selected rows."""
    import peaks_select_common as pc
    pc.check_equality_cases()
    pc.check_rounding_cases()
    logf, freqs = synthetic(pc.EQ_LENGTH)
    for name, s, coeffs, smin, want in pc.equality_cases():
        ref = check(lib, s, logf, freqs, coeffs, 0.1, cap=8, smin=smin)
        assert [list(r[0]) for r in ref] == want, name
    for degree in pc.RND_EACH:
        snrs, logf, freqs, coeffs, smin, r, want = pc.rounding_batch(degree)
        for b in range(2):
            ref = check(lib, snrs[b], logf, freqs, coeffs[b], r, cap=4, smin=smin)
            assert [list(x[0]) for x in ref] == want[b], (degree, b)
            # behind a leading +0.0 coefficient, as poly1d_table stores a trimmed fit
            padded = np.concatenate([np.zeros((coeffs.shape[1], 1)), coeffs[b]], axis=1)
            ref = check(lib, snrs[b], logf, freqs, padded, r, cap=4, smin=smin)
            assert [list(x[0]) for x in ref] == want[b], (degree, b)


def test_peak_finder_inputs_hold_their_conditions():
    """The synthetic S/N PeakFinder's paths are compared on
    (tests/test_gpu_peaks_select.py), against find_peaks alone: lists over
    the cap, within it and empty in the same trial, in both threshold
    branches."""
    import peaks_select_common as pc
    pc.check_finder_case()


def test_invalid_arguments(lib):
    from riptide_amd import _lib
    need = ctypes.c_size_t(123)
    assert lib.rt_find_peaks_workspace_bytes(2, 3000, 3, 64, ctypes.byref(need)) == _lib.RT_OK
    assert need.value >= 2 * 3 * 3000 * 8
    small = ctypes.c_size_t()
    assert lib.rt_find_peaks_workspace_bytes(2, 3000, 3, 0, ctypes.byref(small)) == _lib.RT_OK
    assert 0 < small.value
    assert lib.rt_find_peaks_workspace_bytes(0, 3000, 3, 0, ctypes.byref(small)) == _lib.RT_OK and small.value == 0
    assert lib.rt_find_peaks_workspace_bytes(1, 1 << 32, 3, 0, ctypes.byref(small)) == _lib.RT_EINVAL
    assert b"2^32" in lib.rt_last_error()

    def device(batch=2, length=3000, widths=3, ncoef=1, cap=8, ws=need.value):
        # never reaches a device call: every pointer is NULL
        return lib.rt_find_peaks_device(None, batch, length * widths, length, widths, None, None, None, ncoef, SMIN,
                                        0.1, None, None, None, cap, 64, None, ws, None)

    for kw, text in ((dict(cap=0), b"cap"), (dict(ncoef=0), b"coefficients"),
                     (dict(ws=need.value - 1), b"workspace too small"), (dict(length=1 << 32), b"2^32")):
        assert device(**kw) == _lib.RT_EINVAL, kw
        assert text in lib.rt_last_error(), (kw, lib.rt_last_error())
    assert device(batch=0, ws=0) == _lib.RT_OK
    assert device(widths=0, ws=0) == _lib.RT_OK
    # the host entry point
    one = np.zeros(1)
    assert lib.rt_find_peaks_host(None, 0, 0, None, None, _lib.ptr(one), 1, SMIN, 0.1, None, None, None, 0) \
        == _lib.RT_EINVAL
    assert lib.rt_find_peaks_host(None, 0, 0, None, None, _lib.ptr(one), 0, SMIN, 0.1, None, None, None, 4) \
        == _lib.RT_EINVAL
    assert lib.rt_find_peaks_host(None, 0, 0, None, None, _lib.ptr(one), 1, SMIN, 0.1, None, None, None, 4) \
        == _lib.RT_OK


def test_sanitizer_checker():
    """The walk under AddressSanitizer + UBSan: a stand-alone program
    (`make -C riptide_amd/csrc asan`: build/asan/peaks_check) that calls
    rt_find_peaks_host on heap arrays of exactly the sizes it may touch, with
    a cap below, at and above the cluster counts."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "peaks_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for argv in ((3000, 3, 3, 4, 1), (257, 5, 1, 1, 2), (64, 1, 2, 100, 3), (1, 1, 1, 1, 4), (0, 2, 1, 3, 5)):
        r = subprocess.run([exe] + [str(a) for a in argv], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "runtime error" not in r.stderr, (argv, r.stdout, r.stderr[-3000:])
        assert r.stdout.startswith("clusters "), (argv, r.stdout)
