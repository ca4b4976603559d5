"""Candidate folding (riptide/folding.py:1-81) with the
engine's real-factor downsampling: the series is downsampled by
period / bins / tsamp on the GPU (rt_downsample), cut into whole periods and
scaled exactly as the reference does (numpy, float32); the vertical
downsampling to sub-integrations runs all phase-bin columns in one batched
GPU call (rt_downsample_rows) instead of one call per column.
"""
import numpy as np

from . import _lib
from .libffa import downsample


def downsample_rows(X, factor):
    """Downsample every row of a 2D float32 array by `factor` (one device call)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    rows, n = X.shape
    f = float(factor)
    if not ((f > 1.0) and (f <= n)):
        raise ValueError("Downsampling factor must verify: 1 < f <= size")
    L = _lib.load()
    out = np.empty((rows, int(L.rt_downsampled_size(n, f))), dtype=np.float32)
    if rows:
        _lib.check(L.rt_downsample_rows(_lib.ptr(X), rows, n, f, _lib.ptr(out)))
    return out


def downsample_vertical(X, factor):
    """Downsample a 2D array along its first axis (folding.py:6-16)."""
    m, _ = X.shape
    if not factor > 1:
        raise ValueError("factor must be > 1")
    if not factor < m:
        raise ValueError("factor must be strictly smaller than the number of input lines")
    return np.ascontiguousarray(downsample_rows(np.ascontiguousarray(X.T), factor).T)


def fold(ts, period, bins, subints=None):
    """Fold a TimeSeries at `period` seconds with `bins` phase bins
    (folding.py:19-81): a (subints, bins) array, or (bins,) when the result
    has a single sub-integration."""
    if period > ts.length:
        raise ValueError("Period exceeds data length")
    tbin = period / bins
    if not tbin > ts.tsamp:
        raise ValueError("Bin width is shorter than sampling time")
    if subints is not None:
        subints = int(subints)
        if not subints >= 1:
            raise ValueError("subints must be >= 1 or None")
        full_periods = ts.length / period
        if subints > full_periods:
            raise ValueError(f"subints ({subints}) exceeds the number of signal periods that fit in the data "
                             f"({full_periods})")
    factor = tbin / ts.tsamp
    data = downsample(ts.data, factor)
    m = data.size // bins
    folded = data[:m * bins].reshape(m, bins)
    folded *= (m * factor) ** -0.5
    if subints == 1 or m == 1:
        return folded.sum(axis=0)
    if subints is None or subints == m:
        return folded
    return downsample_vertical(folded, m / subints)


# rt_fold_spec (include/riptide_amd.h)
FOLD_SPEC = np.dtype([("factor", "<f8"), ("out_off", "<u8"), ("series", "<u4"), ("bins", "<u4"),
                      ("subints", "<u4"), ("reserved", "<u4")], align=True)


def check_fold_args(length, tsamp, period, bins, subints):
    """fold()'s argument checks, with its messages, for a series of `length`
    seconds: (downsampling factor, subints as int or None)."""
    if period > length:
        raise ValueError("Period exceeds data length")
    tbin = period / bins
    if not tbin > tsamp:
        raise ValueError("Bin width is shorter than sampling time")
    if subints is not None:
        subints = int(subints)
        if not subints >= 1:
            raise ValueError("subints must be >= 1 or None")
        full_periods = length / period
        if subints > full_periods:
            raise ValueError(f"subints ({subints}) exceeds the number of signal periods that fit in the data "
                             f"({full_periods})")
    return tbin / tsamp, subints


def fold_shape(nsamp, factor, bins, subints):
    """Shape of fold()'s result, from the engine (rt_fold_shape, host only)."""
    import ctypes
    L = _lib.load()
    m, rows = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(L.rt_fold_shape(int(nsamp), float(factor), int(bins), int(subints or 0), ctypes.byref(m),
                               ctypes.byref(rows)))
    return (rows.value, int(bins)) if rows.value else (int(bins),)


def pack_fold_specs(nsamp, length, tsamp, specs):
    """rt_fold_spec table and result shapes of (series, period, bins, subints)
    specs, results packed back to back: (table, shapes, total floats)."""
    table = np.zeros(len(specs), dtype=FOLD_SPEC)
    shapes, off = [], 0
    for k, (series, period, bins, subints) in enumerate(specs):
        bins = int(bins)
        factor, subints = check_fold_args(length, tsamp, period, bins, subints)
        shape = fold_shape(nsamp, factor, bins, subints)
        table[k] = (factor, off, int(series), bins, subints or 0, 0)
        shapes.append(shape)
        off += int(np.prod(shape))
    return table, shapes, off


def fold_many(ts, specs):
    """fold(ts, period, bins, subints) for every (period, bins, subints) of
    `specs`, bit-identical to a loop of fold(): the series is uploaded once
    and every candidate is folded by one batched device call (rt_fold), where
    the loop pays two uploads and two synchronisations per candidate.  A spec
    with bins == 1 (numpy sums a one-column array pairwise, an order the
    kernels do not reproduce) is served by fold().

    One difference from the loop: a period so close to the series length
    that it passes fold()'s checks and still leaves no whole period
    (floor(nsamp / factor) < bins, m == 0) raises ValueError here, as
    rt_fold's contract demands; fold() fails there too, but with the
    ZeroDivisionError of (0 * factor) ** -0.5."""
    specs = [(p, int(b), s) for p, b, s in specs]
    results = [None] * len(specs)
    dev = [k for k, (_, b, _) in enumerate(specs) if b != 1]
    for k, (p, b, s) in enumerate(specs):
        if b == 1:
            results[k] = fold(ts, p, b, s)
    if not dev:
        return results
    data = np.ascontiguousarray(ts.data, dtype=np.float32)
    table, shapes, total = pack_fold_specs(data.size, ts.length, ts.tsamp, [(0,) + specs[k] for k in dev])
    out = np.empty(total, dtype=np.float32)
    L = _lib.load()
    _lib.check(L.rt_fold(_lib.ptr(data), data.size, 1, _lib.ptr(table), len(dev), _lib.ptr(out), out.size))
    for j, k in enumerate(dev):
        o = int(table["out_off"][j])
        results[k] = out[o:o + int(np.prod(shapes[j]))].reshape(shapes[j]).copy()
    return results
