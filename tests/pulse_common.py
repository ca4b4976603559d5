"""Shared by the single-pulse tests: an independent numpy restatement of the
specification (sequential float64 np.cumsum, then plain loops for the centred
maximum and the neighbourhood rule) and the inputs they use."""
import numpy as np

EVENT_DTYPE = np.dtype([("series", np.int32), ("sample", np.int32), ("iwidth", np.int32), ("snr", np.float32)])


def numpy_best(row, widths):
    """(best float32 [N], kbest int32 [N]) of one row."""
    row = np.asarray(row, dtype=np.float32)
    n = row.size
    P = np.concatenate([[0.0], np.cumsum(row.astype(np.float64))])
    best = np.full(n, -np.inf, dtype=np.float32)
    kbest = np.full(n, -1, dtype=np.int32)
    for k, w in enumerate(int(w) for w in widths):
        if w > n:
            continue
        s = ((P[w:] - P[:-w]) / np.sqrt(np.float64(w))).astype(np.float32)     # s[t], 0 <= t <= n - w
        c = w // 2
        centred = np.full(n, -np.inf, dtype=np.float32)
        centred[c:c + s.size] = s
        with np.errstate(invalid="ignore"):
            win = centred > best
        best[win] = centred[win]
        kbest[win] = k
    return best, kbest


def numpy_events_row(best, threshold, radius):
    n = best.size
    out = []
    for t in np.flatnonzero(best >= np.float32(threshold)):
        v = best[t]
        lo = max(0, t - radius)
        if np.all(v > best[lo:t]) and np.all(v >= best[t + 1:t + radius + 1]):
            out.append(int(t))
    return out


def numpy_single_pulse(x, widths, threshold, radius):
    """(events EVENT_DTYPE, best [B, N], kbest [B, N])."""
    x = np.atleast_2d(x)
    bests, kbests, ev = [], [], []
    for b, row in enumerate(x):
        best, kbest = numpy_best(row, widths)
        bests.append(best)
        kbests.append(kbest)
        ev += [(b, t, kbest[t], best[t]) for t in numpy_events_row(best, threshold, int(radius))]
    return np.array(ev, dtype=EVENT_DTYPE), np.stack(bests), np.stack(kbests)


def dyadic_rows(seed, B, N, pulses=()):
    """float32 [B, N], every value an integer / 256 in [-8, 8]: seeded noise
    rounded to that grid, plus boxcar pulses (row, start, width, amplitude)
    added on it (clipped to the row).  Every float64 sum of such values is
    exact in any order."""
    rng = np.random.RandomState(seed)
    x = np.clip(np.round(rng.normal(size=(B, N)) * 256.0) / 256.0, -4.0, 4.0)
    for b, t0, w, a in pulses:
        lo, hi = max(0, t0), min(N, t0 + w)
        if lo < hi:
            x[b % B, lo:hi] += a
    assert np.all(np.abs(x) <= 8.0) and np.all(x * 256.0 == np.round(x * 256.0))
    return x.astype(np.float32)


def gaussian_rows(seed, B, N, pulses=()):
    x = np.random.RandomState(seed).normal(size=(B, N))
    for b, t0, w, a in pulses:
        lo, hi = max(0, t0), min(N, t0 + w)
        if lo < hi:
            x[b % B, lo:hi] += a
    return x.astype(np.float32)


def events_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return (a.shape == b.shape and all(np.array_equal(a[f], b[f]) for f in ("series", "sample", "iwidth"))
            and np.array_equal(a["snr"].view(np.uint32), b["snr"].view(np.uint32)))


def tile_pulses(N, T):
    """Pulses that hang over the row's ends, across the first tile boundary
    and inside (no sample gets more than 4 in all: dyadic rows stay in range)."""
    p = [(2, -3, 9, 1.5), (3, N - 4, 9, 1.5), (0, N // 2, 5, 2.0)]
    if N > T + 8:
        p += [(0, T - 3, 7, 1.75), (1, T - 1, 1, 3.0), (2, T, 1, 3.0), (1, T - 30, 63, 0.75)]
    return p


def run_device(torch, x, widths, thr, R, stream=None, stride_pad=0, **kw):
    """engine.single_pulse_device on the host rows x, optionally as slices of
    a wider tensor (NaN between the rows) and on a side stream.  Returns
    (events EVENT_DTYPE, best, kbest) as host arrays."""
    from riptide_amd import engine
    from riptide_amd.single_pulse import events_to_host
    B, N = x.shape
    if stride_pad:
        wide = torch.full((B, N + stride_pad), float("nan"), dtype=torch.float32, device="cuda")
        wide[:, :N] = torch.from_numpy(x)
        d = wide[:, :N]
        assert d.stride(0) == N + stride_pad
    else:
        d = torch.from_numpy(x).cuda()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    ev, best, kbest = engine.single_pulse_device(d, widths, thr, radius=R, dense=True, stream=stream, **kw)
    if stream is not None:
        stream.synchronize()
    return events_to_host(ev), best.cpu().numpy(), kbest.cpu().numpy()


def assert_same_results(got, ref, what):
    """(events, best, kbest) twice: the same bits."""
    (ev, best, kbest), (rev, rbest, rkbest) = got, ref
    assert best.shape == rbest.shape and kbest.shape == rkbest.shape, what
    bad = np.flatnonzero(best.view(np.uint32).ravel() != rbest.view(np.uint32).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {best.size} best values differ, first at {bad[:5]}"
    bad = np.flatnonzero(kbest.ravel() != rkbest.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {kbest.size} kbest values differ, first at {bad[:5]}"
    assert events_equal(ev, rev), (what, ev.size, rev.size)


def assert_device_is_host(torch, x, widths, thr, R, stream=None, stride_pad=0, numpy_too=False, **kw):
    """best, kbest and the events of the device call equal the host
    specification's, bit for bit, and with numpy_too (dyadic rows only) the
    restatement's above as well.  Returns the host events."""
    from riptide_amd import single_pulse
    got = run_device(torch, x, widths, thr, R, stream=stream, stride_pad=stride_pad, **kw)
    host = single_pulse.single_pulse_host(x, widths, thr, radius=R, dense=True)
    assert_same_results(got, host, "device against the host specification")
    if numpy_too:
        assert_same_results(got, numpy_single_pulse(x, widths, thr, R), "device against the numpy restatement")
    return host[0]
