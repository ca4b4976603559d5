"""Acceleration search by time-domain resampling: a pulsar in a binary is
Doppler-smeared, and for each trial acceleration the dedispersed series is
stretched so that a uniformly accelerated signal becomes strictly periodic;
every stretched series is then searched as usual.

The map is specified once, by the host function resample_host
(rt_resample_host, riptide_amd/csrc/resample_host.hpp); the device form
(engine.resample_device) returns the same bits.  Output row r is source row
src[r] with the float64 factor f = factor[r]:

    q_j = j * (N - j)                           exact integer
    s_j = (int64) rint(f * (double)q_j)         one IEEE double multiply, half-even
    out[r, j] = x[src[r], clamp(j - s_j, 0, N - 1)]

with f = accel * tsamp / (2 c), accel in m/s^2, positive when the source
accelerates away (the observed frequency falls with time).  The shift is zero
at both ends, so the recovered frequency is the mid-observation frequency and
every acceleration trial of one signal lands at the same frequency.  Nearest
neighbour, as peasoup and sigproc resample: a pure gather, so bit-exact.

The searches are EngineSearcher.search_device_accel / search_filterbank_accel
and dispatch.search_filterbank_accel; their peaks are AccelPeak.  Not covered:
acceleration together with the single-pulse search (pulses=), in
build_candidates_filterbank and in refine.  build_candidates folds an
accelerated candidate when its load_series returns TimeSeries.resample(accel).
"""
import typing

import numpy as np

from . import _lib
from .clustering import cluster1d

_L = _lib.load()

C = 299792458.0                  # m/s
MAX_SAMPLES = 1 << 27            # RT_RESAMPLE_MAX_SAMPLES: q_j stays exact in a double
MAX_ROWS = 65535                 # RT_RESAMPLE_MAX_ROWS, of one call


def accel_factor(accel, tsamp):
    """The factor f of the map for an acceleration in m/s^2 and a sampling
    time in seconds: accel * tsamp / (2 c)."""
    return float(accel) * float(tsamp) / (2.0 * C)


def resample_indices(n, factor):
    """The source index of every output sample, int64 [n]: the map restated in
    numpy (np.rint rounds half to even, as rint does)."""
    n = int(n)
    j = np.arange(n, dtype=np.int64)
    s = np.rint(np.float64(factor) * (j * (n - j)).astype(np.float64)).astype(np.int64)
    return np.clip(j - s, 0, max(n - 1, 0))


def resample_rows(nseries, factors, src=None):
    """(src int32 [R], factor float64 [R]) of a resampling call.  src None:
    every row with every factor, row-major [nseries, len(factors)]; otherwise
    one factor per entry of src."""
    f = np.ascontiguousarray(factors, dtype=np.float64).ravel()
    if src is None:
        return np.repeat(np.arange(nseries, dtype=np.int32), f.size), np.tile(f, nseries)
    s = np.asarray(src)
    if s.dtype.kind not in "iu" or s.ndim != 1:
        raise ValueError("src must be a 1-D integer array")
    if s.size != f.size:
        raise ValueError("src and factors must have one entry per output row")
    if s.size and (s.min() < -(1 << 31) or s.max() >= 1 << 31):    # the rest is the entry point's check
        raise ValueError("resample: source row outside [0, B)")
    return np.ascontiguousarray(s, dtype=np.int32), f


def resample_host(data, factors, src=None):
    """The specification on host arrays (rt_resample_host, no device): data
    float32 [N] or [B, N] with unit sample stride (a row-strided view is read
    in place); returns float32 [R, N], the rows of resample_rows(B, factors,
    src)."""
    x = np.asarray(data)
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2 or x.dtype != np.float32:
        raise ValueError("data must be float32 [B, N]")
    B, N = x.shape
    if N and x.strides[1] != 4 or (B > 1 and (x.strides[0] % 4 or x.strides[0] < 4 * N)):
        x = np.ascontiguousarray(x)
    ldx = x.strides[0] // 4 if B > 1 else max(N, 1)
    s, f = resample_rows(B, factors, src)
    out = np.empty((s.size, N), dtype=np.float32)
    _lib.check(_L.rt_resample_host(_lib.ptr(x), B, N, ldx, _lib.ptr(s), _lib.ptr(f), s.size, _lib.ptr(out),
                                   max(N, 1)))
    return out


def accel_step(tobs, smear):
    """The spacing of acceleration trials, m/s^2, for an observation of tobs
    seconds: 16 c smear / tobs^2.  A signal half a step from the nearest trial
    is left with a residual drift a T^2 / (8 c) of `smear` seconds at
    mid-observation."""
    return 16.0 * C * float(smear) / float(tobs) ** 2


def accel_trials(amax, tobs, smear):
    """A symmetric, ascending grid of trial accelerations that contains exactly
    0.0, reaches -amax and +amax, and is spaced by at most accel_step(tobs,
    smear): float64 [2 n + 1], n = ceil(amax / step)."""
    amax = float(amax)
    if not amax >= 0.0 or not np.isfinite(amax):
        raise ValueError("amax must be finite and >= 0")
    step = accel_step(tobs, smear)
    if not step > 0.0:
        raise ValueError("tobs and smear must be > 0")
    n = int(np.ceil(amax / step))
    k = np.arange(-n, n + 1, dtype=np.float64)
    return k * (amax / n) if n else np.zeros(1)


class AccelPeak(typing.NamedTuple):
    """A periodogram peak of one acceleration trial: the fields of
    peak_detection.Peak, then the trial's acceleration in m/s^2.  freq and
    period are those at mid-observation."""
    period: float
    freq: float
    width: int
    ducy: float
    iw: int
    ip: int
    snr: float
    dm: float
    accel: float

    def summary_dict(self):
        return {a: getattr(self, a) for a in ("period", "freq", "dm", "accel", "width", "ducy", "snr")}


def cluster_peaks(peaks, radius, tobs):
    """clustering.cluster_peaks for AccelPeak: the peaks sorted by increasing
    period (a stable sort), then friends-of-friends in frequency with radius
    `radius` / tobs Hz.  Every acceleration trial of one signal has the same
    frequency, so its trials fall into one cluster; the brightest member
    carries the best acceleration.  Returns (sorted peaks, list of clusters)."""
    ps = sorted((p if isinstance(p, AccelPeak) else AccelPeak(*p) for p in peaks), key=lambda p: p.period)
    if not ps:
        return ps, []
    ids = cluster1d(np.asarray([p.freq for p in ps]), radius / tobs, already_sorted=True)
    return ps, [[ps[i] for i in cl] for cl in ids]
