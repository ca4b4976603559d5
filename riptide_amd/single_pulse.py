"""Single-pulse search of the DM trials: boxcar S/N at a ladder of widths, the
centred best width of every sample, local maxima above a threshold (the
events), and the events of all DMs clustered into pulses.

The arithmetic is specified once, by the host function single_pulse_host
(rt_single_pulse_host, riptide_amd/csrc/pulse_host.hpp); the device form
(engine.single_pulse_device) returns the same bits.  The series are assumed
dereddened and normalised to unit variance (engine.deredden_normalise), so a
boxcar sum over sqrt(width) is a signal-to-noise ratio.
"""
import ctypes

import numpy as np

from . import _lib
from .clustering import cluster1d

_L = _lib.load()

# rt_pulse_event (include/riptide_amd.h)
EVENT_DTYPE = np.dtype([("series", np.int32), ("sample", np.int32), ("iwidth", np.int32), ("snr", np.float32)])


def generate_pulse_widths(wmax, factor=1.5):
    """Ascending integer widths in samples 1, 2, 3, 4, 6, 9, 13, ... up to
    wmax: each is max(previous + 1, floor(previous * factor))."""
    wmax = int(wmax)
    if wmax < 1:
        raise ValueError("wmax must be >= 1")
    if not factor > 1.0:
        raise ValueError("factor must be > 1")
    widths = [1]
    while True:
        w = max(widths[-1] + 1, int(np.floor(widths[-1] * float(factor))))
        if w > wmax:
            break
        widths.append(w)
    return np.asarray(widths, dtype=np.int32)


def single_pulse_host(data, widths, threshold, radius=None, dense=False):
    """The specification on host arrays (rt_single_pulse_host, no device):
    data float32 [N] or [B, N] with unit sample stride (a row-strided view is
    read in place), widths ascending, radius in samples (default: the largest
    width).  Returns the events as a structured array of EVENT_DTYPE sorted by
    (series, sample), and with dense=True (events, best, kbest): float32 and
    int32 [B, N]."""
    x = np.asarray(data)
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2 or x.dtype != np.float32:
        raise ValueError("data must be float32 [B, N]")
    B, N = x.shape
    if N and x.strides[1] != 4 or (B > 1 and (x.strides[0] % 4 or x.strides[0] < 4 * N)):
        x = np.ascontiguousarray(x)
    ldx = x.strides[0] // 4 if B > 1 else max(N, 1)
    w = np.ascontiguousarray(widths, dtype=np.int32).ravel()
    if not w.size:
        raise ValueError("single pulse: no trial widths")
    radius = int(w.max() if radius is None else radius)
    if radius < 0:
        raise ValueError("radius must be >= 0")
    best = np.empty((B, N), dtype=np.float32) if dense else None
    kbest = np.empty((B, N), dtype=np.int32) if dense else None
    count = ctypes.c_uint64()
    cap = 1024
    while True:
        ev = np.empty(cap, dtype=EVENT_DTYPE)
        _lib.check(_L.rt_single_pulse_host(_lib.ptr(x), B, N, ldx, _lib.ptr(w), w.size, float(threshold), radius,
                                           _lib.ptr(ev), cap, ctypes.byref(count),
                                           _lib.ptr(best) if dense else None, _lib.ptr(kbest) if dense else None))
        if count.value <= cap:
            break
        cap = int(count.value)
    ev = ev[:count.value]
    return (ev, best, kbest) if dense else ev


class SinglePulse:
    """One pulse: the highest-S/N event of a cluster of events in time and DM.
    time (s) and sample are the centre of the best boxcar, width is in
    samples, npoints the number of events of the cluster, dm_lo / dm_hi the
    range of trial DMs they cover."""
    __slots__ = ("time", "sample", "dm", "idm", "width", "snr", "npoints", "dm_lo", "dm_hi")

    def __init__(self, time, sample, dm, idm, width, snr, npoints, dm_lo, dm_hi):
        self.time = float(time)
        self.sample = int(sample)
        self.dm = float(dm)
        self.idm = int(idm)
        self.width = int(width)
        self.snr = float(snr)
        self.npoints = int(npoints)
        self.dm_lo = float(dm_lo)
        self.dm_hi = float(dm_hi)

    def to_dict(self):
        return {k: getattr(self, k) for k in self.__slots__}

    @classmethod
    def from_dict(cls, items):
        return cls(*(items[k] for k in cls.__slots__))

    def __eq__(self, other):
        return isinstance(other, SinglePulse) and self.to_dict() == other.to_dict()

    def __repr__(self):
        return ("SinglePulse(time={time:.6f}, sample={sample}, dm={dm:.3f}, idm={idm}, width={width}, snr={snr:.2f}, "
                "npoints={npoints}, dm_lo={dm_lo:.3f}, dm_hi={dm_hi:.3f})").format(**self.to_dict())


def cluster_events(events, dms, tsamp, time_radius=None, dm_gap=1, widths=None):
    """Group the events of every DM trial into pulses, on the host.

    events: EVENT_DTYPE records whose `series` is the index into `dms`;
    widths: the trial widths of the search, which `iwidth` indexes (default:
    generate_pulse_widths(512), the default of the searches).  Events
    are grouped in time (clustering.cluster1d of sample * tsamp, radius
    time_radius seconds; default: the largest width); a group is split where
    its sorted DM indices are more than dm_gap apart.  One SinglePulse per
    group, from its highest-S/N event (ties: the lower DM index, then the
    earlier sample).  Returns the pulses sorted by decreasing S/N (ties: DM
    index, then sample)."""
    events = np.asarray(events, dtype=EVENT_DTYPE)
    dms = np.asarray(dms, dtype=np.float64)
    widths = np.asarray(generate_pulse_widths(512) if widths is None else widths, dtype=np.int64)
    if not events.size:
        return []
    if time_radius is None:
        time_radius = float(widths.max()) * float(tsamp)
    times = events["sample"].astype(np.float64) * float(tsamp)
    pulses = []
    for group in cluster1d(times, float(time_radius)):
        group = group[np.argsort(events["series"][group], kind="stable")]
        idm = events["series"][group].astype(np.int64)
        cuts = np.flatnonzero(np.diff(idm) > int(dm_gap)) + 1
        for part in np.split(group, cuts):
            ev = events[part]
            order = np.lexsort((ev["sample"], ev["series"], -ev["snr"].astype(np.float64)))
            top = ev[order[0]]
            i = int(top["series"])
            pulses.append(SinglePulse(time=int(top["sample"]) * float(tsamp), sample=int(top["sample"]),
                                      dm=dms[i], idm=i, width=int(widths[int(top["iwidth"])]),
                                      snr=float(top["snr"]), npoints=len(part),
                                      dm_lo=dms[int(ev["series"].min())], dm_hi=dms[int(ev["series"].max())]))
    pulses.sort(key=lambda p: (-p.snr, p.idm, p.sample))
    return pulses


def _default_widths(widths, n):
    if widths is None:
        return generate_pulse_widths(min(512, int(n)))
    return np.ascontiguousarray(widths, dtype=np.int32).ravel()


def events_to_host(events, series_offset=0):
    """engine.PulseEvents (device columns) as one EVENT_DTYPE array, `series`
    shifted by series_offset."""
    out = np.empty(int(events.series.numel()), dtype=EVENT_DTYPE)
    out["series"] = events.series.cpu().numpy() + int(series_offset)
    out["sample"] = events.sample.cpu().numpy()
    out["iwidth"] = events.iwidth.cpu().numpy()
    out["snr"] = events.snr.cpu().numpy()
    return out


def search_pulses(series, tsamp, dms, widths=None, threshold=8.0, radius=None, time_radius=None, dm_gap=1,
                  max_events=1 << 20, stream=None):
    """Single-pulse search of a device batch [B, N] that is already
    dereddened and normalised, row b at trial DM dms[b].  widths default to
    generate_pulse_widths(512).  Returns (pulses, events): the SinglePulse
    list of cluster_events and the EVENT_DTYPE records on the host."""
    from . import engine
    if series.dim() == 1:
        series = series.unsqueeze(0)
    if len(dms) != series.shape[0]:
        raise ValueError("one DM per series")
    w = _default_widths(widths, series.shape[1])
    ev = engine.single_pulse_device(series, w, threshold, radius=radius, max_events=max_events, stream=stream)
    events = events_to_host(ev)
    return cluster_events(events, dms, tsamp, time_radius=time_radius, dm_gap=dm_gap, widths=w), events


def search_filterbank_pulses(fb_or_fname, dms, deredden_params, widths=None, threshold=8.0, mask=None, zero_dm=False,
                             kdm=None, nout=None, batch=8, device=None, radius=None, time_radius=None, dm_gap=1,
                             max_events=1 << 20, block_mask=None, cutouts=None, inject=None):
    """Single-pulse search of a channelised SIGPROC file (a file name, a
    reading.Filterbank or PackedFilterbank) at the trial DMs without leaving
    the device: dedispersion.dedisperse_filterbank, then slices of `batch` DMs
    through engine.deredden_normalise (deredden_params: rmed_width in
    seconds, rmed_minpts) and engine.single_pulse_device, one download of the
    events and cluster_events.  mask, zero_dm, kdm, nout, block_mask, inject:
    as for dispatch.search_filterbank (cutouts are read back from the file as
    it is, without the injected signals: injection.inject_filterbank writes a
    file that has them).  Returns (pulses, events); `series` of an
    event is its index into dms.

    cutouts: None, or a dict of keyword arguments of
    pulse_candidates.build_pulse_candidates (an empty one for its defaults;
    mask, zero_dm, block_mask, kdm and device default to this call's).  The
    function then returns (pulses, events, candidates): one PulseCandidate per
    pulse, in the order of pulses, with the frequency-time and DM-time cutouts
    read back from the file."""
    from . import engine
    from .dedispersion import KDM
    from .dispatch import _dedispersed
    from .reading import Filterbank, open_filterbank
    fb = fb_or_fname if isinstance(fb_or_fname, Filterbank) else open_filterbank(fb_or_fname)
    kdm = KDM if kdm is None else float(kdm)
    dms = [float(d) for d in dms]
    if not dms:
        none = [], np.empty(0, dtype=EVENT_DTYPE)
        return none if cutouts is None else none + ([],)
    parts = []
    with _dedispersed(fb, dms, device, max(1, int(batch)), mask=mask, nout=nout, kdm=kdm, zero_dm=zero_dm,
                      block_mask=block_mask, inject=inject) as (series, _, slices):
        w = _default_widths(widths, series.shape[1])
        ws = int(round(deredden_params["rmed_width"] / fb.tsamp))
        for b0, b1 in slices:
            x = engine.deredden_normalise(series[b0:b1], ws, deredden_params["rmed_minpts"])
            ev = engine.single_pulse_device(x, w, threshold, radius=radius, max_events=max_events)
            parts.append((b0, ev))
        events = np.concatenate([events_to_host(ev, b0) for b0, ev in parts])
    pulses = cluster_events(events, dms, fb.tsamp, time_radius=time_radius, dm_gap=dm_gap, widths=w)
    if cutouts is None:
        return pulses, events
    from .pulse_candidates import build_pulse_candidates
    kwargs = dict(mask=mask, zero_dm=zero_dm, block_mask=block_mask, kdm=kdm, device=device)
    kwargs.update(cutouts)
    return pulses, events, build_pulse_candidates(fb, pulses, **kwargs)
