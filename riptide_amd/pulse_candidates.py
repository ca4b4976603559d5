"""Single-pulse candidates from the filterbank: for every pulse of a
single-pulse search the dedispersed frequency-time cutout (is the pulse
broadband, and straight at its DM?) and the DM-time "bow-tie" (does the S/N
peak at a non-zero DM and fall off on both sides?), the two arrays a person
inspects and a classifier takes as input.

Both are batches of one primitive, a dedispersed and time-decimated window of
a resident block (engine.pulse_cutouts_device; the kernel:
csrc/cutout_kernels.hip), specified once by pulse_cutouts_host
(rt_pulse_cutouts_host): the device returns the same bits.  This is the
single-pulse counterpart of candidate.build_candidates_filterbank.
"""
import ctypes

import numpy as np

from . import _lib
from .dedispersion import (DEFAULT_GULP_BYTES, KDM, _checked_mask, _checked_sample_type, _gulp_layout, _host_block,
                           _upload_block_mask, band_edges, dispersion_delays)
from .engine import CUTOUT_JOB_DTYPE, DEDISP_ZERO_DM, checked_cutout_jobs
from .single_pulse import SinglePulse

_L = _lib.load()


class PulseCandidate:
    """A single pulse with its two diagnostic cutouts.

    pulse       the SinglePulse
    freq_time   float32 [B, T]: B sub-bands dedispersed at the pulse's DM, T
                bins of `factor` samples, the pulse in bin T // 2
    dm_time     float32 [K, T]: the whole band dedispersed at the K DMs `dms`
    dms         float64 [K]
    band_freqs  float64 [B]: the mean channel frequency of every band (MHz)
    factor      samples summed per bin
    t0, tbin    time of bin 0 at the highest frequency and the length of a
                bin, in seconds (t0 is negative for a window that starts
                before the file)
    """
    __slots__ = ("pulse", "freq_time", "dm_time", "dms", "band_freqs", "factor", "t0", "tbin")

    def __init__(self, pulse, freq_time, dm_time, dms, band_freqs, factor, t0, tbin):
        self.pulse = pulse
        self.freq_time = np.asarray(freq_time, dtype=np.float32)
        self.dm_time = np.asarray(dm_time, dtype=np.float32)
        self.dms = np.asarray(dms, dtype=np.float64)
        self.band_freqs = np.asarray(band_freqs, dtype=np.float64)
        self.factor = int(factor)
        self.t0 = float(t0)
        self.tbin = float(tbin)

    @staticmethod
    def _robust_rows(a):
        """Every row minus its median, over 1.4826 * its median absolute
        deviation; a row whose deviation is zero is left centred."""
        a = np.asarray(a, dtype=np.float64)
        c = a - np.median(a, axis=1, keepdims=True)
        s = 1.4826 * np.median(np.abs(c), axis=1, keepdims=True)
        return np.where(s > 0, c / np.where(s > 0, s, 1.0), c).astype(np.float32)

    def normalised(self):
        """A copy whose freq_time and dm_time rows are robustly normalised
        (host numpy): each row minus its median, divided by 1.4826 times its
        median absolute deviation, so noise has about unit variance; a row
        with a deviation of zero is only centred."""
        return PulseCandidate(self.pulse, self._robust_rows(self.freq_time), self._robust_rows(self.dm_time), self.dms,
                              self.band_freqs, self.factor, self.t0, self.tbin)

    def to_dict(self):
        items = {k: getattr(self, k) for k in self.__slots__}
        items["pulse"] = self.pulse.to_dict()
        return items

    @classmethod
    def from_dict(cls, items):
        items = dict(items)
        items["pulse"] = SinglePulse.from_dict(items["pulse"])
        return cls(*(items[k] for k in cls.__slots__))

    def __repr__(self):
        return (f"PulseCandidate({self.pulse!r}, freq_time={self.freq_time.shape}, dm_time={self.dm_time.shape}, "
                f"factor={self.factor})")


class CutoutPlan:
    """What cutout_jobs lays out for a list of pulses: `jobs` (CUTOUT_JOB_DTYPE,
    `start` in samples of the file), pulse p owning the jobs [p * (nbands +
    ndm), (p + 1) * (nbands + ndm)) -- first its nbands frequency-time rows,
    then its ndm DM-time rows -- and the floats [p, p + 1) * (nbands + ndm) *
    nbins of the output; `delays` int32 [npulses * (1 + ndm), nchans], pulse
    p's rows being p * (1 + ndm) (its own DM) and the ndm that follow (its DM
    grid); `max_delay`; `dms` float64 [npulses, ndm]; `factors` and `starts`
    int64 [npulses]; `bands` uint32 [nbands, 2]; nbins, nbands, ndm."""

    def __init__(self, jobs, delays, max_delay, dms, factors, starts, bands, nbins):
        self.jobs, self.delays, self.max_delay, self.dms = jobs, delays, int(max_delay), dms
        self.factors, self.starts, self.bands, self.nbins = factors, starts, bands, int(nbins)
        self.nbands, self.ndm = bands.shape[0], dms.shape[1]

    @property
    def npulses(self):
        return self.starts.size

    @property
    def rows_per_pulse(self):
        return self.nbands + self.ndm

    def spans(self, nsamp):
        """int64 [npulses, 2]: the rows [lo, hi) of a file of nsamp samples
        that pulse p's windows read (lo == hi: none)."""
        R = 1 + self.ndm
        top = self.delays.reshape(self.npulses, R, -1).max(axis=(1, 2)).astype(np.int64) if self.npulses else 0
        lo = np.clip(self.starts, 0, nsamp)
        hi = np.clip(self.starts + self.nbins * self.factors + top, lo, nsamp)
        return np.stack([lo, hi], axis=1).astype(np.int64).reshape(-1, 2)


def cutout_jobs(pulses, freqs, tsamp, nbins=256, nbands=64, ndm=64, dm_span=None, factor=None, kdm=KDM):
    """The CutoutPlan of the frequency-time and DM-time cutouts of `pulses`
    (SinglePulse records) in a file of channel frequencies `freqs` (MHz).

    Per pulse the decimation is f = max(1, width // 2) samples per bin (or
    `factor` for every pulse) and the window starts at sample - (nbins * f) //
    2, so the pulse falls in bin nbins // 2.  The frequency-time rows are the
    `nbands` bands of dedispersion.band_edges at the pulse's DM.  The DM-time
    rows are the whole band at `ndm` DMs evenly spaced from max(dm - dm_span,
    0) to dm + dm_span: the grid is clipped at DM 0.  dm_span defaults to the
    DM offset whose delay across the band equals half the window,

      (nbins * f / 2) * tsamp / (kdm * (fmin ** -2 - fmax ** -2)),

    so that the bow-tie just fills the cutout (0 for a single frequency).  The
    delays are dedispersion.dispersion_delays'.

    nbins = 256, nbands = 64 and ndm = 64 are defaults of the interface, sizes
    a diagnostic plot or a classifier input commonly has; they are not tuned
    values, and nothing in the kernel prefers them."""
    freqs = np.ascontiguousarray(np.atleast_1d(freqs), dtype=np.float64)
    nchans = freqs.size
    nbins, ndm = int(nbins), int(ndm)
    if nbins < 1 or ndm < 1:
        raise ValueError("nbins and ndm must be at least 1")
    if factor is not None and int(factor) < 1:
        raise ValueError("factor must be at least 1")
    if dm_span is not None and not float(dm_span) >= 0.0:
        raise ValueError("dm_span must be non-negative")
    bands = band_edges(nchans, nbands)
    nbands = bands.shape[0]
    P = len(pulses)
    sweep = float(kdm) * (freqs.min() ** -2 - freqs.max() ** -2)
    factors = np.array([max(1, p.width // 2) if factor is None else int(factor) for p in pulses], dtype=np.int64)
    starts = np.array([p.sample for p in pulses], dtype=np.int64) - (nbins * factors) // 2
    dms = np.empty((P, ndm), dtype=np.float64)
    for i, p in enumerate(pulses):
        span = dm_span
        if span is None:
            span = (nbins * factors[i] / 2) * float(tsamp) / sweep if sweep > 0 else 0.0
        dms[i] = np.linspace(max(p.dm - float(span), 0.0), p.dm + float(span), ndm) if ndm > 1 else p.dm
    R = 1 + ndm
    if P:
        trial = np.concatenate([np.array([[p.dm] for p in pulses], dtype=np.float64), dms], axis=1).ravel()
        delays, max_delay = dispersion_delays(freqs, trial, tsamp, kdm)
        delays = delays.astype(np.int32)
    else:
        delays, max_delay = np.empty((0, nchans), dtype=np.int32), 0
    jobs = np.zeros(P * (nbands + ndm), dtype=CUTOUT_JOB_DTYPE).reshape(P, nbands + ndm)
    jobs["start"] = starts[:, None]
    jobs["factor"] = factors[:, None]
    jobs["nbins"] = nbins
    jobs["out_off"] = np.arange(P * (nbands + ndm), dtype=np.uint64).reshape(P, nbands + ndm) * np.uint64(nbins)
    row0 = np.arange(P, dtype=np.int64)[:, None] * R
    jobs["delay_row"][:, :nbands] = row0
    jobs["band_lo"][:, :nbands] = bands[:, 0]
    jobs["band_hi"][:, :nbands] = bands[:, 1]
    jobs["delay_row"][:, nbands:] = row0 + 1 + np.arange(ndm)
    jobs["band_lo"][:, nbands:] = 0
    jobs["band_hi"][:, nbands:] = nchans
    return CutoutPlan(jobs.ravel(), delays, max_delay, dms, factors, starts, bands, nbins)


def _host_mask_struct(block_mask, data_dtype, nbits, nchans, t_origin):
    """(rt_block_mask, the arrays it points to) of a rfi.BlockMask for host
    data; (None, None) for None."""
    if block_mask is None:
        return None, None
    cells = np.ascontiguousarray(np.asarray(block_mask.cells).astype(bool), dtype=np.uint8)
    if cells.ndim != 2 or cells.shape[1] != nchans:
        raise ValueError(f"the block mask's cells must be [nblocks, {nchans}]")
    fill = np.ascontiguousarray(block_mask.typed_fill(data_dtype, nbits))
    if not 0 <= int(t_origin) < 1 << 64 or int(block_mask.block_len) < 1:
        raise ValueError("block_len must be at least 1 and t_origin in [0, 2^64)")
    bm = _lib.BlockMaskStruct(cells.ctypes.data, cells.shape[0], int(block_mask.block_len), int(t_origin),
                              fill.ctypes.data)
    return bm, (cells, fill)


def pulse_cutouts_host(data, jobs, delays, max_delay, mask=None, zero_dm=False, nbits=None, block_mask=None,
                       t_origin=0, out=None):
    """The specification on the host (rt_pulse_cutouts_host, no device): data
    [nsamp, nchans] uint8, int8 or float32 (with nbits packed rows, as for
    dedispersion.dedisperse_host), jobs an array of engine.CUTOUT_JOB_DTYPE
    whose `start` is relative to row 0 of data, delays [R, nchans] (clamped to
    [0, max_delay]), block_mask a rfi.BlockMask with t_origin the absolute
    sample of row 0.  Returns float32 [max(out_off + nbins)] (or `out`, a
    float32 array at least that long): engine.pulse_cutouts_device's
    definition, sample by sample in channel order."""
    data, code, nsamp, nchans = _host_block(data, nbits)
    jobs = checked_cutout_jobs(jobs)
    delays = np.ascontiguousarray(delays, dtype=np.int32)
    if delays.ndim != 2 or delays.shape[1] != nchans:
        raise ValueError("delays must be [R, nchans]")
    mask = _checked_mask(mask, nchans)
    bm, keep = _host_mask_struct(block_mask, data.dtype, nbits, nchans, t_origin)
    need = int((jobs["out_off"] + jobs["nbins"]).max()) if jobs.size else 0
    if out is None:
        out = np.zeros(need, dtype=np.float32)
    elif out.dtype != np.float32 or out.ndim != 1 or not out.flags.c_contiguous or out.size < need:
        raise ValueError(f"out must be a contiguous float32 array of at least {need}")
    _lib.check(_L.rt_pulse_cutouts_host(_lib.ptr(data), code, nsamp, nchans, _lib.ptr(delays), delays.shape[0],
                                        int(max_delay), None if mask is None else _lib.ptr(mask), _lib.ptr(jobs),
                                        jobs.size, _lib.ptr(out), out.size, DEDISP_ZERO_DM if zero_dm else 0,
                                        None if bm is None else ctypes.byref(bm)))
    del keep
    return out


def plan_chunks(spans, row_bytes, chunk_bytes, names=None):
    """Pack pulses into contiguous row ranges of the file: spans int64
    [npulses, 2] of the rows [lo, hi) each pulse reads.  The pulses are sorted
    by their first row (ties: their index) and packed greedily: a pulse joins
    the current range while the range, extended to the pulse's last row, stays
    within chunk_bytes of input (row_bytes per row).  Returns a list of (lo,
    hi, indices): every pulse with a non-empty span is in exactly one chunk,
    which covers its span.  ValueError, naming the pulse (names[i], or its
    index), when one pulse's own span exceeds chunk_bytes."""
    spans = np.asarray(spans, dtype=np.int64).reshape(-1, 2)
    cap = int(chunk_bytes) // int(row_bytes)
    chunks = []
    for i in np.lexsort((np.arange(len(spans)), spans[:, 0])):
        lo, hi = int(spans[i, 0]), int(spans[i, 1])
        if hi <= lo:
            continue
        if hi - lo > cap:
            who = names[i] if names is not None else f"pulse {i}"
            raise ValueError(f"{who} reads {hi - lo} rows of {row_bytes} bytes, more than chunk_bytes = "
                             f"{int(chunk_bytes)}: raise chunk_bytes, or cut its window (nbins, dm_span)")
        if chunks and max(chunks[-1][1], hi) - chunks[-1][0] <= cap:
            chunks[-1][1] = max(chunks[-1][1], hi)
            chunks[-1][2].append(int(i))
        else:
            chunks.append([lo, hi, [int(i)]])
    return [(lo, hi, idx) for lo, hi, idx in chunks]


def build_pulse_candidates(fb_or_fname, pulses, nbins=256, nbands=64, ndm=64, dm_span=None, factor=None, kdm=None,
                           mask=None, zero_dm=False, block_mask=None, chunk_bytes=DEFAULT_GULP_BYTES, device=None):
    """PulseCandidates of a list of SinglePulse records, in their order,
    straight from the channelised file (a name for reading.open_filterbank, or
    a Filterbank / PackedFilterbank).  nbins, nbands, ndm, dm_span, factor and
    kdm: cutout_jobs.  mask, zero_dm, block_mask (a rfi.BlockMask): as for
    dispatch.search_filterbank.

    The pulses are sorted by the first row of the file they read and packed
    into contiguous row ranges of at most chunk_bytes of input (plan_chunks).
    A chunk is uploaded once (a packed file stays packed), transposed once,
    and all of its pulses' rows come from one launch
    (engine.pulse_cutouts_device) and one download.  The result does not depend
    on chunk_bytes.  A window that runs past either end of the file gets no
    contribution from there.  ValueError when a single pulse's rows exceed
    chunk_bytes."""
    import torch
    from . import engine
    from ._args import resolve_device
    from .reading import Filterbank, open_filterbank
    fb = fb_or_fname if isinstance(fb_or_fname, Filterbank) else open_filterbank(fb_or_fname)
    pulses = list(pulses)
    if not pulses:
        return []
    nbits = _checked_sample_type(fb)
    kdm = KDM if kdm is None else float(kdm)
    plan = cutout_jobs(pulses, fb.freqs, fb.tsamp, nbins=nbins, nbands=nbands, ndm=ndm, dm_span=dm_span,
                       factor=factor, kdm=kdm)
    mask = _checked_mask(mask, fb.nchans)
    row_elems, dtype = _gulp_layout(fb)
    spans = plan.spans(fb.nsamp)
    chunks = plan_chunks(spans, row_elems * dtype.itemsize, chunk_bytes, names=[repr(p) for p in pulses])
    J, R, T = plan.rows_per_pulse, 1 + plan.ndm, plan.nbins
    jobs = plan.jobs.reshape(len(pulses), J)
    delays = plan.delays.reshape(len(pulses), R, fb.nchans)
    result = np.zeros((len(pulses), J, T), dtype=np.float32)   # a pulse that reads no row stays zero
    dev = resolve_device(device)
    with torch.cuda.device(dev):
        d_mask = None if mask is None else torch.from_numpy(mask).to(dev)
        d_bm = _upload_block_mask(fb, block_mask, dev, max((hi for _, hi, _ in chunks), default=0))
        for lo, hi, idx in chunks:
            block = torch.from_numpy(np.array(fb.data[lo:hi])).to(dev)
            cj = jobs[idx].copy()
            cj["start"] -= lo
            cj["delay_row"] = (np.arange(len(idx), dtype=np.uint32)[:, None] * R
                               + (cj["delay_row"] - cj["delay_row"][:, :1]))
            cj["out_off"] = np.arange(cj.size, dtype=np.uint64).reshape(cj.shape) * np.uint64(T)
            cd = delays[idx].reshape(-1, fb.nchans)
            out = engine.pulse_cutouts_device(block, cj.ravel(), torch.from_numpy(cd).to(dev),
                                              int(cd.max()) if cd.size else 0, mask=d_mask, zero_dm=zero_dm,
                                              nbits=nbits, block_mask=d_bm, t_origin=lo)
            result[idx] = out.cpu().numpy().reshape(len(idx), J, T)
    band_freqs = np.array([fb.freqs[a:b].mean() for a, b in plan.bands])
    return [PulseCandidate(p, result[i, :plan.nbands], result[i, plan.nbands:], plan.dms[i], band_freqs,
                           plan.factors[i], plan.starts[i] * fb.tsamp, plan.factors[i] * fb.tsamp)
            for i, p in enumerate(pulses)]
