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
