"""Peak clustering on the GPU: rt_find_peaks_device (find_peaks_chunk_kernel +
find_peaks_join_kernel) against rt_find_peaks_host, exact in counts, rows and
S/N bits, for every chunk size; the chunk joins at their boundary cases;
truncation; PeakFinder and EngineSearcher with device_cluster on against off.

The seeded inputs, the numpy restatement and the host wrapper are those of
tests/test_peaks_cluster_host.py.
"""
import ctypes

import numpy as np
import pytest

import test_peaks_cluster_host as ph
from test_peaks_cluster_host import CANARY_ROW, CANARY_SNR, SMIN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from riptide_amd import _lib
    return _lib.load()


def device_find(lib, snrs, logf, freqs, coeffs, smin, r, cap, chunk_rows, pad=5):
    """rt_find_peaks_device on snrs [B, L, W] uploaded at a stride of L * W +
    pad floats, the outputs prefilled with canaries (8 more slots after the
    last column): (counts [B, W], rows [B, W, cap], snr [B, W, cap])."""
    import torch
    from riptide_amd import _lib
    snrs = np.ascontiguousarray(snrs, dtype=np.float32)
    B, L, W = snrs.shape
    stride = L * W + pad
    host = np.full((B, stride), np.float32(1e9))          # a stray read of the padding would be selected
    host[:, :L * W] = snrs.reshape(B, -1)
    d_snrs = torch.from_numpy(host).cuda()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    d = [torch.from_numpy(np.array(a, dtype=np.float64)).cuda() for a in (logf, freqs, coeffs)]
    need = ctypes.c_size_t()
    assert lib.rt_find_peaks_workspace_bytes(B, L, W, chunk_rows, ctypes.byref(need)) == 0
    ws = torch.full((need.value + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((B * W + 8,), -1, dtype=torch.int32, device="cuda")
    rows = torch.from_numpy(np.full(B * W * cap + 8, CANARY_ROW, dtype=np.uint32).view(np.int32)).cuda()
    out = torch.full((B * W * cap + 8,), float(CANARY_SNR), dtype=torch.float32, device="cuda")
    rc = lib.rt_find_peaks_device(_lib.ptr(d_snrs), B, stride, L, W, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]),
                                  coeffs.shape[-1], smin, r, _lib.ptr(counts), _lib.ptr(rows), _lib.ptr(out), cap,
                                  chunk_rows, _lib.ptr(ws), need.value, None)
    assert rc == 0, lib.rt_last_error()
    torch.cuda.synchronize()
    counts, rows, out = counts.cpu().numpy(), rows.cpu().numpy().view(np.uint32), out.cpu().numpy()
    assert (ws[need.value:].cpu().numpy() == 0xA5).all(), "workspace overrun"
    assert (counts[B * W:] == -1).all() and (rows[B * W * cap:] == CANARY_ROW).all()
    assert (out[B * W * cap:] == CANARY_SNR).all()
    return (counts[:B * W].astype(np.int64).reshape(B, W), rows[:B * W * cap].reshape(B, W, cap),
            out[:B * W * cap].reshape(B, W, cap))


def assert_device_is_host(lib, snrs, logf, freqs, coeffs, r, cap, chunk_rows, smin=SMIN):
    """Every trial of the batch: the device's arrays equal the host walk's,
    canaries past the records included.  Returns the host counts [B, W]."""
    snrs = np.asarray(snrs, dtype=np.float32)
    coeffs = np.asarray(coeffs, dtype=np.float64)
    counts, rows, out = device_find(lib, snrs, logf, freqs, coeffs, smin, r, cap, chunk_rows)
    host_counts = []
    for b in range(snrs.shape[0]):
        hc, hr, ho = ph.host_find(lib, snrs[b], logf, freqs, coeffs[b], smin, r, cap)
        assert np.array_equal(counts[b], hc), (b, counts[b], hc)
        assert np.array_equal(rows[b], hr), b
        assert np.array_equal(out[b].view(np.uint32), ho.view(np.uint32)), b
        host_counts.append(hc)
    return np.array(host_counts)


@pytest.mark.parametrize("ncoef", [1, 3])
@pytest.mark.parametrize("chunk_rows", [64, 256, 1000, 0])
@pytest.mark.parametrize("length", sorted(ph.SEEDS))
def test_device_matches_host(lib, length, chunk_rows, ncoef):
    cases = [ph.random_case(length, seed, ncoef) for seed in ph.SEEDS[length]]      # B = 2: the trials differ
    _, logf, freqs, _, r = cases[0]
    snrs = np.stack([c[0] for c in cases])
    coeffs = np.stack([c[3] * (1.0 + 0.01 * b) for b, c in enumerate(cases)])       # and so do their thresholds
    for b in range(2):      # the honesty condition, on the restatement alone
        ref = ph.ref_trial(snrs[b], logf, freqs, coeffs[b], SMIN, r)
        assert ph.honest_enough(ref), (length, b)
    assert_device_is_host(lib, snrs, logf, freqs, coeffs, r, cap=length, chunk_rows=chunk_rows)


def test_more_widths_than_a_group(lib):
    """W = 37: a second workgroup column of 5 widths (32 widths per group),
    and waves with 10, 9, 9, 9 widths between them."""
    cases = [ph.random_case(257, seed, 1) for seed in ph.SEEDS[257]]
    _, logf, freqs, _, r = cases[0]
    rng = np.random.RandomState(3)
    snrs = np.stack([np.concatenate([np.roll(c[0], k, axis=0) for k in rng.randint(0, 257, size=13)], axis=1)[:, :37]
                     for c in cases])
    coeffs = np.full((2, 37, 1), SMIN)
    hc = assert_device_is_host(lib, snrs, logf, freqs, coeffs, r, cap=16, chunk_rows=64)
    assert (hc >= 1).all() and len(np.unique(hc)) > 2


# ---- constructed cases at chunk_rows = 64 on the grid f = 1 + k / 4 (rising)
def boundary_columns(length=300):
    """{name: (column spikes, radius, expected peak rows)}"""
    r = 0.25
    run = {i: 8.0 for i in range(60, 201)}
    cases = {
        # row 63 ends a cluster, row 65 is 0.5 away: just above r = 0.5 - 1 ulp, equal to r = 0.5
        "gap_above": ({62: 9.0, 63: 8.0, 65: 10.0, 66: 8.5}, np.nextafter(0.5, 0.0), [62, 65]),
        "gap_equal": ({62: 9.0, 63: 8.0, 65: 10.0, 66: 8.5}, 0.5, [65]),
        # rows 63 and 64 adjacent across the boundary
        "adjacent_split": ({63: 9.0, 64: 8.0}, np.nextafter(0.25, 0.0), [63, 64]),
        "adjacent_joined": ({63: 8.0, 64: 9.0}, 0.25, [64]),
        # one cluster over rows 60-200 (chunks 1 and 2 wholly inside), its maximum in each part
        "span_max_first": ({**run, 61: 20.0}, r, [61]),
        "span_max_middle": ({**run, 130: 20.0}, r, [130]),
        "span_max_last": ({**run, 199: 20.0}, r, [199]),
        # the same maximum in two chunks: the earlier row (rising grid)
        "span_tie": ({**run, 70: 20.0, 150: 20.0}, r, [70]),
        "span_tie_all": (run, r, [60]),
        # two selected rows 130 apart, an empty chunk between them
        "far_joined": ({10: 9.5, 140: 9.0}, 32.5, [10]),
        "far_split": ({10: 9.0, 140: 9.5}, np.nextafter(32.5, 0.0), [10, 140]),
        # chunk 1 entirely one selected run
        "whole_chunk": ({i: 8.0 + (i == 100) for i in range(64, 128)}, r, [100]),
        # selected rows only in the last, partial chunk
        "last_partial": ({length - 3: 9.0, length - 1: 9.5}, r, [length - 3, length - 1]),
    }
    return cases


@pytest.mark.parametrize("rising", [True, False])
def test_chunk_boundaries(lib, rising):
    """All constructed columns in one launch per radius, W = their number.
    On the falling grid (a periodogram's own direction) the later of two
    equal maxima wins, as np.argmax over cluster1d's ascending frequencies."""
    length = 300
    logf, freqs = ph.synthetic(length, rising)
    cases = boundary_columns(length)
    for radius in sorted({c[1] for c in cases.values()}):
        names = [k for k, c in cases.items() if c[1] == radius]
        s = np.zeros((2, length, len(names)), dtype=np.float32)
        for iw, k in enumerate(names):
            for i, v in cases[k][0].items():
                s[0, i, iw] = v
                s[1, length - 1 - i, iw] = v        # trial 1: the mirrored column
        coeffs = np.full((2, len(names), 1), SMIN)
        ref = ph.ref_trial(s[0], logf, freqs, coeffs[0], SMIN, radius)
        for iw, k in enumerate(names):
            want = cases[k][2]
            if not rising and k == "span_tie":
                want = [150]
            if not rising and k == "span_tie_all":
                want = [200]
            assert list(ref[iw][0]) == want, (k, list(ref[iw][0]))
        hc = assert_device_is_host(lib, s, logf, freqs, coeffs, radius, cap=8, chunk_rows=64)
        assert [int(c) for c in hc[0]] == [len(cases[k][2]) for k in names]


def test_truncation(lib):
    """cap = 4, 9 clusters in one column and 2 in its neighbour: the count of
    9, the first 4 records, the neighbour and every slot past the records
    (assert_device_is_host compares whole arrays, canaries included)."""
    logf, freqs = ph.synthetic(700)
    s = np.zeros((2, 700, 2), dtype=np.float32)
    s[0, 30:690:80, 0] = np.arange(9, dtype=np.float32) + 8.0
    s[0, [100, 500], 1] = 9.0
    s[1, [100, 500], 0] = 9.0
    s[1, 30:690:80, 1] = np.arange(9, dtype=np.float32) + 8.0
    coeffs = np.full((2, 2, 1), SMIN)
    for chunk_rows in (64, 0):
        hc = assert_device_is_host(lib, s, logf, freqs, coeffs, 0.25, cap=4, chunk_rows=chunk_rows)
        assert hc.tolist() == [[9, 2], [2, 9]]
    counts, rows, out = device_find(lib, s, logf, freqs, coeffs, SMIN, 0.25, 4, 64)
    assert rows[0, 0].tolist() == [30, 110, 190, 270] and out[0, 0].tolist() == [8.0, 9.0, 10.0, 11.0]
    assert rows[0, 1].tolist() == [100, 500, CANARY_ROW, CANARY_ROW]


@pytest.mark.parametrize("chunk_rows", [64, 0])
def test_threshold_equality_and_rounding(lib, chunk_rows):
    """The device twin of test_peaks_cluster_host's test of the same name:
    S/N equal to the threshold or to smin, and polynomials for which a fused
    multiply-add changes the comparison (peak_threshold's __dadd_rn(__dmul_rn())
    on the device), in both directions."""
    import peaks_select_common as pc
    pc.check_equality_cases()
    pc.check_rounding_cases()
    logf, freqs = ph.synthetic(pc.EQ_LENGTH)
    for name, s, coeffs, smin, want in pc.equality_cases():
        hc = assert_device_is_host(lib, s[None], logf, freqs, coeffs[None], 0.1, cap=8, chunk_rows=chunk_rows,
                                   smin=smin)
        assert hc[0].tolist() == [len(w) for w in want], name
        _, rows, _ = device_find(lib, s[None], logf, freqs, coeffs[None], smin, 0.1, 8, chunk_rows)
        assert [rows[0, iw, :len(w)].tolist() for iw, w in enumerate(want)] == want, name
    for degree in pc.RND_EACH:
        snrs, logf, freqs, coeffs, smin, r, want = pc.rounding_batch(degree)
        hc = assert_device_is_host(lib, snrs, logf, freqs, coeffs, r, cap=4, chunk_rows=chunk_rows, smin=smin)
        assert hc.tolist() == [[len(w) for w in trial] for trial in want], degree
        _, rows, _ = device_find(lib, snrs, logf, freqs, coeffs, smin, r, 4, chunk_rows)
        assert [[i] for i in rows[0, :, 0].tolist()] == want[0], degree


def test_empty_shapes(lib):
    """length 0 zeroes the counts; batch or widths of 0 launch nothing."""
    import torch
    from riptide_amd import _lib
    counts = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    one = torch.zeros(8, dtype=torch.float64, device="cuda")
    rc = lib.rt_find_peaks_device(None, 2, 0, 0, 3, None, None, _lib.ptr(one), 1, SMIN, 0.1, _lib.ptr(counts), None,
                                  None, 4, 0, None, 0, None)
    assert rc == 0, lib.rt_last_error()
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [0] * 6


# ---- the Python layer
@pytest.fixture(scope="module")
def small_search():
    """2^16 samples, periods 0.1-1 s, 240-260 bins, a pulsar in both trials:
    (plan, tobs, device S/N [2, L, W])."""
    import torch
    from riptide_amd import TimeSeries, engine
    n, tsamp = 1 << 16, 256e-6
    np.random.seed(5)
    x = np.stack([TimeSeries.generate(n * tsamp, tsamp, period, amplitude=amp, ducy=0.05).data
                  for period, amp in ((0.31, 25.0), (0.47, 18.0))]).astype(np.float32)
    plan = engine.PeriodogramPlan.for_search(n, tsamp, 0.1, 1.0, 240, 260, ducy_max=0.2)
    return plan, n * tsamp, plan.run(torch.from_numpy(x).cuda())


@pytest.mark.parametrize("max_peaks", [4096, 1])
def test_peak_finder_device_cluster(small_search, max_peaks):
    """PeakFinder(device_cluster=True) returns the default path's (peaks,
    polycos), peak order included; with max_peaks = 1 every column of more
    than one cluster takes the truncated-column path."""
    from riptide_amd.peaks import PeakFinder
    plan, tobs, snr = small_search
    want = PeakFinder(plan, tobs)(snr, dms=[0.0, 5.0])
    got = PeakFinder(plan, tobs, device_cluster=True, max_peaks=max_peaks)(snr, dms=[0.0, 5.0])
    assert len(want) == len(got) == 2
    per_width = {}
    for b in range(2):
        assert got[b][0] == want[b][0], b
        assert len(want[b][0]) >= 2, "the pulsar and its harmonics give several peaks"
        assert sorted(got[b][1]) == sorted(want[b][1])
        for iw in want[b][1]:
            assert np.array_equal(np.asarray(got[b][1][iw]), np.asarray(want[b][1][iw])), (b, iw)
        for p in want[b][0]:
            per_width[b, p.iw] = per_width.get((b, p.iw), 0) + 1
    assert max(per_width.values()) >= 2, "a column of several clusters (the truncated path at max_peaks = 1)"


def test_engine_searcher_device_cluster(monkeypatch):
    """EngineSearcher(device_cluster=True) against the default on two fake
    series; None reads RIPTIDE_AMD_DEVICE_PEAKS."""
    import riptide_amd as rt
    from riptide_amd.dispatch import EngineSearcher, Trial
    tobs, tsamp = 32.0, 256e-6
    dered = {"rmed_width": 5.0, "rmed_minpts": 101}
    ranges = [{"name": "short", "ffa_search": {"period_min": 0.2, "period_max": 1.0, "bins_min": 240, "bins_max": 260},
               "find_peaks": {"smin": 7.0}}]
    np.random.seed(9)
    trials = [Trial(data=rt.TimeSeries.generate(tobs, tsamp, period, amplitude=amp, ducy=0.03).data.astype(np.float32),
                    tsamp=tsamp, metadata={"dm": dm})
              for period, amp, dm in ((0.4, 20.0, 0.0), (0.73, 15.0, 10.0))]
    want = EngineSearcher(dered, ranges, device=0, batch=2, device_cluster=False)(trials)
    got = EngineSearcher(dered, ranges, device=0, batch=2, device_cluster=True)(trials)
    assert [len(p) for p in want] == [len(p) for p in got] and all(len(p) >= 1 for p in want)
    assert got == want
    monkeypatch.delenv("RIPTIDE_AMD_DEVICE_PEAKS", raising=False)
    assert EngineSearcher(dered, ranges).device_cluster is False
    monkeypatch.setenv("RIPTIDE_AMD_DEVICE_PEAKS", "1")
    assert EngineSearcher(dered, ranges).device_cluster is True
    assert EngineSearcher(dered, ranges, device_cluster=False).device_cluster is False
