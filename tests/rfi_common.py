"""Shared by the RFI tests: the numpy restatement of the zero-DM filter
(RT_DEDISP_ZERO_DM in include/riptide_amd.h) and its bounds.

  S[t]      = sum over unmasked c of x[t, c]    (8-bit: int64, exact; float32:
                                                 float64, ascending channels)
  m[t]      = float32(S[t] / Nu)                (float64 division)
  ref[d, t] = sum over unmasked c of (float64(x) - float64(m))[t + delay, c]
"""
import numpy as np


def keep_of(mask, nchans):
    return np.ones(nchans, dtype=bool) if mask is None else ~np.asarray(mask, dtype=bool)


def numpy_zero_dm_mean(x, mask=None):
    """float32 [nsamp]: bit for bit what the host and the device give for
    8-bit data; for float32 data the host's (ascending channel order)."""
    keep = keep_of(mask, x.shape[1])
    nu = int(keep.sum())
    if nu == 0:
        return np.zeros(x.shape[0], dtype=np.float32)
    if x.dtype == np.float32:
        s = np.zeros(x.shape[0], dtype=np.float64)
        for c in np.flatnonzero(keep):
            s += x[:, c].astype(np.float64)
    else:
        s = x[:, keep].astype(np.int64).sum(axis=1).astype(np.float64)
    return (s / np.float64(nu)).astype(np.float32)


def numpy_zero_dm_dedisperse(x, m32, delays, nout, mask=None):
    """(ref64 [ndm, nout], sum |y| [ndm, nout], sum |m| [ndm, nout]) in float64,
    y = float64(x) - float64(m32) exactly."""
    keep = keep_of(mask, x.shape[1])
    ndm = delays.shape[0]
    m = m32.astype(np.float64)
    ref, mag, magm = (np.zeros((ndm, nout), dtype=np.float64) for _ in range(3))
    for d in range(ndm):
        for c in np.flatnonzero(keep):
            k = int(delays[d, c])
            y = x[k:k + nout, c].astype(np.float64) - m[k:k + nout]
            ref[d] += y
            mag[d] += np.abs(y)
            magm[d] += np.abs(m[k:k + nout])
    return ref, mag, magm


def zero_dm_bound(x, delays, mag, magm):
    """8-bit: nchans * 2^-24 * sum |y| (m and so y are reproducible; float32
    summation in channel order).  float32 input: (nchans + 2) * 2^-24 * sum |y|
    + 2^-22 * sum |m|: m is free by one float32 ulp (another summation order
    of the float64 sum), doubled to absorb the second-order terms."""
    nchans = delays.shape[1]
    if x.dtype == np.float32:
        return (nchans + 2) * 2.0 ** -24 * mag + 2.0 ** -22 * magm
    return nchans * 2.0 ** -24 * mag


def assert_zero_dm_dedispersed(out, x, delays, nout, mask=None):
    """out against the restatement, within zero_dm_bound; returns (largest
    error, largest bound) for a test that wants to print them."""
    m32 = numpy_zero_dm_mean(x, mask)
    ref, mag, magm = numpy_zero_dm_dedisperse(x, m32, delays, nout, mask)
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == ref.shape, (out.dtype, out.shape, ref.shape)
    assert np.all(np.isfinite(out))
    err = np.abs(out.astype(np.float64) - ref)
    bound = zero_dm_bound(x, delays, mag, magm)
    assert np.all(err <= bound), f"max excess {float((err - bound).max()):.3e} (max err {float(err.max()):.3e})"
    return float(err.max()), float(bound.max())
