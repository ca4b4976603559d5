"""Shared by the DM plan tests: the numpy restatement of the planner's
quantities and of the decimated dedispersion specification
(rt_dedisperse_ds_host), and the sample types and delay tables they use."""
import numpy as np

import dedisp_common as dc

KDM = dc.KDM
KINDS = ("uint8", "int8", "float32", "u1", "u2", "u4", "u16")


def plan_quantities(freqs, kdm=KDM):
    """(kdisp, ksmear) of a band as include/riptide_amd.h defines them, in the
    same float64 operations."""
    freqs = np.asarray(freqs, dtype=np.float64)
    fmin, fmax = freqs.min(), freqs.max()
    cw = (fmax - fmin) / float(freqs.size - 1)
    flo, fhi = fmin - cw / 2.0, fmax + cw / 2.0
    fmid = (flo + fhi) / 2.0
    a, b = fmid - cw / 2.0, fmid + cw / 2.0
    kdisp = kdm * (1.0 / (flo * flo) - 1.0 / (fhi * fhi))
    ksmear = kdm * (1.0 / (a * a) - 1.0 / (b * b))
    return kdisp, ksmear


def smear(dms, ksmear, wmin):
    return np.maximum(wmin, ksmear * np.asarray(dms, dtype=np.float64))


def numpy_zero_dm_mean(vals, mask=None):
    """m[t] = float32(S[t] / Nu): S exact for integers, float64 in ascending
    channel order for float32 data (the host's order)."""
    keep = np.ones(vals.shape[1], dtype=bool) if mask is None else ~np.asarray(mask, dtype=bool)
    nu = int(keep.sum())
    if not nu:
        return np.zeros(vals.shape[0], dtype=np.float32)
    if vals.dtype.kind in "iu":
        s = vals[:, keep].astype(np.int64).sum(axis=1).astype(np.float64)
    else:
        s = np.zeros(vals.shape[0], dtype=np.float64)
        for c in np.flatnonzero(keep):
            s = s + vals[:, c].astype(np.float64)
    return (s / np.float64(nu)).astype(np.float32)


def numpy_decimate(vals, f, mean=None):
    """z float32 [nsamp // f, nchans]: per output a float32 accumulator from
    +0.0 that takes one float32 addition per sample, in index order; with the
    zero-DM mean series the addend is float32(x) - mean[t]."""
    nz = vals.shape[0] // f
    x32 = vals[:nz * f].astype(np.float32)
    if mean is not None:
        x32 = x32 - mean[:nz * f, None]
        assert x32.dtype == np.float32
    z = np.zeros((nz, vals.shape[1]), dtype=np.float32)
    for i in range(f):
        z = z + x32[i::f]
        assert z.dtype == np.float32
    return z


def numpy_dedisperse_ds(vals, delays, f, nout, mask=None, zero_dm=False):
    """The specification restated: decimation first, the sum second, both in
    float32 from +0.0 in index order.  vals [nsamp, nchans] are the sample
    values (after any block mask); delays are in decimated samples."""
    mean = numpy_zero_dm_mean(vals, mask) if zero_dm else None
    z = numpy_decimate(vals, f, mean)
    return dc.numpy_dedisperse_f32(z, delays, nout, mask)


def delay_table(ndm, nchans, spread, base=3):
    """int64 [ndm, nchans]: channel c of DM d at base + c % 5 + d * spread //
    (ndm - 1) * (c + 1) // nchans -- within a tile of 16 DMs the last
    channel's delays span about `spread` samples."""
    d = np.arange(ndm)[:, None]
    c = np.arange(nchans)[None, :]
    return (base + c % 5 + (d * spread // max(ndm - 1, 1)) * (c + 1) // nchans).astype(np.int64)


# ---- the end-to-end fixture: a dispersed pulse train in a 64-channel 8-bit file
E2E = dict(nchans=64, nsamp=1 << 17, tsamp=256e-6, fch1=400.0, foff=-100.0 / 64, period=0.5, width=16, amp=6.0)
E2E_DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}
E2E_RANGES = [{"name": "short",
               "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
               "find_peaks": {"smin": 7.0}}]


def e2e_freqs():
    return E2E["fch1"] + E2E["foff"] * np.arange(E2E["nchans"])


def e2e_plan():
    """DM 2.5 to 12 at wmin 1 ms: a step at the file's 256 us, one at f = 2
    and one at f = 4 (the smearing of DM 10 is 3 ms)."""
    from riptide_amd.dedispersion import dm_plan
    return dm_plan(e2e_freqs(), E2E["tsamp"], dm_max=12.0, dm_min=2.5, wmin=1e-3)


def e2e_true_dm(plan):
    """(index of the plan trial nearest DM 10, the injected DM a little off it)."""
    k = int(np.argmin(np.abs(plan.dms - 10.0)))
    return k, float(plan.dms[k]) + 0.02


def e2e_data(dm):
    """uint8 [nsamp, nchans]: noise of sigma 12 around 128 plus a train of
    boxcar pulses, 16 samples (4 ms: 4 samples at f = 4) wide, period 0.5 s,
    delayed per channel by the dispersion formula at `dm`."""
    rng = np.random.RandomState(42)
    nsamp, nchans, tsamp = E2E["nsamp"], E2E["nchans"], E2E["tsamp"]
    x = rng.normal(128.0, 12.0, size=(nsamp, nchans))
    delays = dc.numpy_delays(e2e_freqs(), [dm], tsamp)[0]
    t = np.arange(nsamp)
    for c in range(nchans):
        phase = ((t - delays[c]) * tsamp) % E2E["period"]
        x[(t >= delays[c]) & (phase < E2E["width"] * tsamp), c] += E2E["amp"]
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def e2e_header():
    return {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": E2E["tsamp"],
            "nbits": 8, "fch1": E2E["fch1"], "foff": E2E["foff"], "nchans": E2E["nchans"], "nifs": 1}


def e2e_period_step():
    """One trial step of the search at the injected period P: the FFA's period
    step there is tau * P / T with tau the bin width, at most P / bins_min, so
    at most P^2 / (bins_min * T) over the whole observation T."""
    tobs = E2E["nsamp"] * E2E["tsamp"]
    return E2E["period"] ** 2 / (E2E_RANGES[0]["ffa_search"]["bins_min"] * tobs)
