"""Shared by the pulse-cutout tests: the definition of riptide_amd.h restated in
plain numpy, seeded inputs of every sample type, and job tables."""
import numpy as np

from dedisp_common import kind_samples, numpy_zero_dm_mean

from riptide_amd.engine import CUTOUT_JOB_DTYPE

KINDS = ("uint8", "int8", "float32", "u1", "u2", "u4", "u16")
FLOAT_KINDS = ("float32", "u16")


def make_jobs(rows):
    """CUTOUT_JOB_DTYPE from (start, factor, nbins, delay_row, band_lo,
    band_hi) tuples, the outputs laid out one after the other."""
    jobs = np.zeros(len(rows), dtype=CUTOUT_JOB_DTYPE)
    off = 0
    for j, (start, f, T, row, lo, hi) in zip(jobs, rows):
        j["start"], j["factor"], j["nbins"], j["delay_row"], j["band_lo"], j["band_hi"] = start, f, T, row, lo, hi
        j["out_off"] = off
        off += T
    return jobs


def replaced(vals, block_mask, t_origin, fill):
    """x' of riptide_amd.h: vals [nsamp, nchans] with the flagged cells' samples
    set to fill[c] (fill already in the sample's type)."""
    t = (int(t_origin) + np.arange(vals.shape[0])) // block_mask.block_len
    return np.where(block_mask.cells[t], np.asarray(fill)[None, :], vals).astype(vals.dtype)


def numpy_cutouts(vals, jobs, delays, max_delay, float_sum, mask=None, mean=None):
    """float32 [sum of nbins]: every job of the definition.  vals [nsamp,
    nchans] are the values the samples stand for.  Integer sums (float_sum
    False) are exact in int64 and converted once; float sums keep one float32
    accumulator per bin that starts at +0.0 and takes one float32 addition per
    sample, channels ascending and within a channel j ascending; with `mean`
    (the zero-DM series) a sample is float32(x) - mean[t] first."""
    nsamp, nchans = vals.shape
    out = np.zeros(int((jobs["out_off"] + jobs["nbins"]).max()) if jobs.size else 0, dtype=np.float32)
    delays = np.clip(np.asarray(delays, dtype=np.int64), 0, int(max_delay))
    v32 = vals.astype(np.float32)
    for job in jobs:
        T, f = int(job["nbins"]), int(job["factor"])
        n = np.arange(T, dtype=np.int64)
        if float_sum or mean is not None:
            acc = np.zeros(T, dtype=np.float32)
        else:
            acc = np.zeros(T, dtype=np.int64)
        for c in range(int(job["band_lo"]), int(job["band_hi"])):
            if mask is not None and mask[c]:
                continue
            first = int(job["start"]) + n * f + int(delays[int(job["delay_row"]), c])
            for j in range(f):
                t = first + j
                ok = (t >= 0) & (t < nsamp)
                if not ok.any():
                    continue
                tt = t[ok]
                if mean is not None:
                    acc[ok] = acc[ok] + (v32[tt, c] - mean[tt])
                elif float_sum:
                    acc[ok] = acc[ok] + v32[tt, c]
                else:
                    acc[ok] += vals[tt, c].astype(np.int64)
        out[int(job["out_off"]):int(job["out_off"]) + T] = acc.astype(np.float32)
    return out


def case_samples(seed, nsamp, nchans, kind, exact_floats=False):
    """(data for the entry points, values [nsamp, nchans], nbits) of a kind.
    exact_floats: float32 data holds small integers (the zero-DM mean's float64
    sum is then exact in any order)."""
    rng = np.random.RandomState(seed)
    if kind == "float32" and exact_floats:
        x = rng.randint(-40, 41, size=(nsamp, nchans)).astype(np.float32)
        return x, x, None
    return kind_samples(rng, nsamp, nchans, kind)


def zero_dm_mean(vals, mask):
    """The zero-DM series of integer-valued samples (float32 ones included)."""
    return numpy_zero_dm_mean(vals.astype(np.int64) if vals.dtype.kind == "f" else vals, mask)


def edge_jobs(nsamp, nchans, R):
    """Jobs at every edge of a block of nsamp rows: the windows the definition
    clamps, the bands it allows, factors of one sample up to a bin longer than
    a tile of bins."""
    C = nchans
    return make_jobs([
        (0, 1, 257, 0, 0, C),                   # the whole band, two tiles
        (-37, 3, 65, 1 % R, 0, C),              # starts before the block
        (nsamp - 90, 7, 64, 2 % R, 0, C),       # runs past its end
        (nsamp + 3, 2, 63, 0, 0, C),            # wholly behind the block: zeros
        (-5000, 5, 10, 1 % R, 0, C),            # wholly in front of it: zeros
        (nsamp - 70, 1, 64, 2 % R, 0, C),       # start + delay crosses the end for the delayed channels only
        (100, 4, 5, 0, C // 2, C // 2),         # an empty band
        (100, 2, 256, 1 % R, C // 3, C),        # a band
        (90, 2, 256, 1 % R, 0, max(C // 2, 1)), # one overlapping it
        (11, 300, 9, 2 % R, 0, C),              # a bin longer than a tile of bins
        (5, 64, 33, 0, 0, C),
        (7, 1, 1, 1 % R, 0, C),                 # one bin
    ])
