"""Shared by the dedispersion tests: the numpy restatement they compare
against, the band they use and the float32 bound."""
import numpy as np

KDM = 1.0 / 2.41e-4
TSAMP = 1e-3


def band(nchans, ascending=False):
    """nchans channel centres of a 368-400 MHz band; DM 50 spans about 230
    samples of 1 ms across it."""
    step = 32.0 / nchans
    return 368.0 + step * np.arange(nchans) if ascending else 400.0 - step * np.arange(nchans)


def numpy_delays(freqs, dms, tsamp, kdm=KDM):
    freqs = np.asarray(freqs, dtype=np.float64)
    f_ref = freqs.max()
    out = np.zeros((len(dms), freqs.size), dtype=np.int64)
    for d, dm in enumerate(dms):
        for c, f in enumerate(freqs):
            a = 1.0 / (f * f) - 1.0 / (f_ref * f_ref)
            out[d, c] = int(np.floor(kdm * float(dm) * a / tsamp + 0.5))
    return out


def numpy_dedisperse(x, delays, nout, mask=None):
    """(float64 sums [ndm, nout], float64 sums of |x|): exact for 8-bit data."""
    ndm, nchans = delays.shape
    acc = np.zeros((ndm, nout), dtype=np.float64)
    mag = np.zeros((ndm, nout), dtype=np.float64)
    for d in range(ndm):
        for c in range(nchans):
            if mask is not None and mask[c]:
                continue
            col = x[delays[d, c]:delays[d, c] + nout, c].astype(np.float64)
            acc[d] += col
            mag[d] += np.abs(col)
    return acc, mag


def assert_dedispersed(out, x, delays, nout, mask=None):
    """Bit for bit for 8-bit data; |out - ref64| <= nchans * 2^-24 * sum |x|
    (recursive summation in float32) for float data."""
    ref, mag = numpy_dedisperse(x, delays, nout, mask)
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == ref.shape, (out.dtype, out.shape, ref.shape)
    if x.dtype == np.float32:
        assert np.all(np.isfinite(out))
        err = np.abs(out.astype(np.float64) - ref)
        bound = delays.shape[1] * 2.0 ** -24 * mag
        assert np.all(err <= bound), f"max excess {float((err - bound).max()):.3e}"
    else:
        assert np.array_equal(out, ref.astype(np.float32)), \
            f"{int((out != ref.astype(np.float32)).sum())} of {out.size} sums differ"


def samples(rng, nsamp, nchans, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return rng.normal(size=(nsamp, nchans)).astype(np.float32)
    info = np.iinfo(dtype)
    return rng.randint(info.min, info.max + 1, size=(nsamp, nchans)).astype(dtype)
