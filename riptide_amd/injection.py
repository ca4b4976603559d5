"""Synthetic pulsars and single pulses injected into filterbank data, on the
raw block as it sits in device memory, in front of everything else
(rt_inject_* in include/riptide_amd.h, the kernel in csrc/inject_kernels.hip,
DESIGN.md section 5g).

The device does integer arithmetic and a table gather, nothing else: a signal
is a float32 template (a pulse profile over 2^log2bins phase bins, or a pulse
window of L samples), per-channel amplitudes and per-channel delays, and for
absolute sample t and channel c

  u  = t - delay[c]
  ue = u + rint(f * u * (span - u))            (f = 0: ue = u)
  periodic:  value = amp[c] * tmpl[(phase0 + ue * step) >> (64 - log2bins)]
  pulse:     value = amp[c] * tmpl[ue - t0]    inside the window, else 0

with the phase a 64-bit count of 2^-64 turns that wraps by itself.  The
signals' values are summed in float32 in the order given and added to the
sample; an 8-bit sample takes floor(sum + r) with r in [0, 1) a hash of (seed,
t, c): stochastic rounding, unbiased, so a signal far below one count per
sample survives, and a function of the absolute sample alone, so the result
does not depend on how the file is cut into gulps.  The float64 physics --
profiles, spectral weights, delays, the amplitude that gives the requested
S/N -- lives here, in injection_tables.

Limits.  Packed 1-, 2-, 4- and 16-bit files are refused: deliberately out of
scope.  One template per signal: no per-channel smearing or scattering.  The
acceleration term u + s(u) is the first-order inverse of the search's
resampling out[j] = x[j - s_j]: resampled at the same acceleration the train
is periodic up to a residual of at most (|f| * span)^2 * span / 4 + 1 samples,
not exactly.  `snr` is the matched-filter S/N of the series dedispersed at the
true DM, at the true period and acceleration, with no mask and no filter in
front: what a search reports is lower.

Entry points that do not take inject= (candidate.build_candidates_filterbank,
pulse_candidates.build_pulse_candidates, rfi.*) read the file as it is: write
an injected copy with inject_filterbank and run them on that.
"""
import typing
from fractions import Fraction

import numpy as np

from . import _lib
from .dedispersion import KDM, _checked_data, _checked_sample_type, dispersion_delays
from .engine import DEDISP_DTYPES, INJECT_SPEC_DTYPE

_L = _lib.load()
_check = _lib.check

__all__ = ["PulsarSignal", "PulseSignal", "InjectionTables", "injection_tables", "inject_host", "inject_filterbank"]

MAX_SPAN = 1 << 27          # RT_RESAMPLE_MAX_SAMPLES
_CHUNK = 1 << 20            # samples of one numpy pass of the normalisation
_FWHM = 2.0 * np.sqrt(2.0 * np.log(2.0))


class PulsarSignal(typing.NamedTuple):
    """A periodic signal: period in seconds (at mid-observation when
    accelerated), dm in pc cm^-3, snr as defined in the module docstring, a
    von Mises profile of duty cycle ducy (FWHM in turns, libffa.generate_signal's
    kappa) peaking at phase phi0 at sample 0, accel in m/s^2 (positive: the
    source accelerates away; acceleration.accel_factor), flux proportional to
    frequency ** spectral_index, a template of 2 ** log2bins phase bins."""
    period: float
    dm: float
    snr: float
    ducy: float = 0.02
    phi0: float = 0.5
    accel: float = 0.0
    spectral_index: float = 0.0
    log2bins: int = 10


class PulseSignal(typing.NamedTuple):
    """One dispersed pulse: time in seconds at infinite frequency, dm in
    pc cm^-3, snr as defined in the module docstring, a Gaussian of FWHM
    `width` seconds, flux proportional to frequency ** spectral_index."""
    time: float
    dm: float
    snr: float
    width: float
    spectral_index: float = 0.0


class InjectionTables:
    """What the injection entry points take: the signal table `specs`
    (engine.INJECT_SPEC_DTYPE, one record per signal) and the packed arrays
    its offsets point into -- `tmpl` and `amp` float32, `delay` int32 -- with
    the `signals` they were built from, `nchans` and `span`.  Checked on
    construction (rt_inject_check's table and value checks)."""

    def __init__(self, specs, tmpl, amp, delay, nchans, signals=(), span=0):
        specs = np.asarray(specs)
        if specs.dtype != INJECT_SPEC_DTYPE or specs.ndim != 1:
            raise ValueError("specs must be a one-dimensional array of engine.INJECT_SPEC_DTYPE records")
        self.specs = np.ascontiguousarray(specs)
        self.tmpl = np.ascontiguousarray(tmpl, dtype=np.float32).ravel()
        self.amp = np.ascontiguousarray(amp, dtype=np.float32).ravel()
        self.delay = np.ascontiguousarray(delay, dtype=np.int32).ravel()
        self.nchans = int(nchans)
        self.signals = tuple(signals)
        self.span = int(span)
        self._device = {}
        self.check("uint8", 0, 0)

    def check(self, dtype, nsamp, t_origin):
        """ValueError unless a block of `nsamp` rows of `dtype` samples from
        absolute sample t_origin can take these tables (rt_inject_check)."""
        name = str(np.dtype(dtype).name) if not isinstance(dtype, str) else dtype
        if name not in ("uint8", "int8", "float32"):
            raise ValueError("inject: the sample type must be uint8, int8 or float32 (packed rows are refused)")
        if int(t_origin) < 0:
            raise ValueError("inject: t_origin must not be negative")
        _check(_L.rt_inject_check(DEDISP_DTYPES[name], int(nsamp), self.nchans, int(t_origin), _lib.ptr(self.specs),
                                  self.specs.size, _lib.ptr(self.tmpl), self.tmpl.size, _lib.ptr(self.amp),
                                  self.amp.size, _lib.ptr(self.delay), self.delay.size))

    def on_device(self, device):
        """(specs as bytes, tmpl, amp, delay) as tensors on `device`, uploaded
        on first use and kept."""
        import torch
        key = (device.type, device.index)
        if key not in self._device:
            def up(a):
                # never an empty allocation: the entry point wants pointers
                return torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(device)
            self._device[key] = (up(self.specs.view(np.uint8)), up(self.tmpl), up(self.amp), up(self.delay))
        return self._device[key]

    def __len__(self):
        return self.specs.size

    def __repr__(self):
        return f"InjectionTables({self.specs.size} signals, nchans={self.nchans}, span={self.span})"


def _signal_index(spec, u):
    """The template entry of one record of a signal table at the delay-free
    samples u (int64 array): the integer map of the specification in numpy.
    For a pulse an entry outside [0, length) means no signal."""
    u = np.asarray(u, dtype=np.int64)
    with np.errstate(over="ignore"):
        ue = u
        if float(spec["factor"]) != 0.0:
            q = u * (np.int64(spec["span"]) - u)
            ue = u + np.rint(np.float64(spec["factor"]) * q.astype(np.float64)).astype(np.int64)
        if int(spec["kind"]) == 0:
            ph = np.uint64(spec["phase0"]) + ue.astype(np.uint64) * np.uint64(spec["step"])
            return (ph >> np.uint64(64 - int(spec["log2bins"]))).astype(np.int64)
        return ue - np.int64(spec["t0"])


def _realised_norm(spec, tmpl, span):
    """sqrt(sum over t in [0, span) of tmpl[index(t)]^2) at zero delay, float64."""
    total = 0.0
    t64 = tmpl.astype(np.float64)
    for a in range(0, span, _CHUNK):
        idx = _signal_index(spec, np.arange(a, min(a + _CHUNK, span), dtype=np.int64))
        if int(spec["kind"]) == 1:
            idx = idx[(idx >= 0) & (idx < t64.size)]
        total += float(np.sum(t64[idx] ** 2))
    return np.sqrt(total)


def _turns(x):
    """round(2^64 * x) mod 2^64 for a float x, exactly."""
    return int(round(Fraction(float(x)) * (1 << 64))) % (1 << 64)


def injection_tables(signals, freqs, tsamp, span, sigma, kdm=KDM):
    """The InjectionTables of `signals` (PulsarSignal / PulseSignal, or one of
    them) for channel frequencies `freqs` (MHz, the file's order), sampling
    time tsamp, and a dedispersed series of `span` samples: the length the
    search works on (nsamp minus the DM list's largest delay), which is both
    the N of the acceleration map and the stretch the S/N is defined over.
    sigma is the per-channel noise standard deviation, a scalar or [nchans]
    (rfi.channel_stats(fb).std).

    Amplitudes: channel c gets A * w_c with w_c = (f_c / f_ref) ** alpha
    normalised to sum 1 (f_ref the mean frequency) and A such that
    sqrt(sum_t s_t^2) / sqrt(sum_c sigma_c^2) == snr, s_t = A * tmpl[index(t)]
    over t in [0, span) at zero delay -- the realised samples, evaluated with
    the integer map itself.  ValueError for a signal that leaves nothing inside
    [0, span), a period not above 2 * tsamp, and whatever rt_inject_check
    refuses."""
    from .acceleration import accel_factor
    if isinstance(signals, (PulsarSignal, PulseSignal)):
        signals = [signals]
    signals = list(signals)
    freqs = np.ascontiguousarray(np.atleast_1d(freqs), dtype=np.float64)
    nchans = freqs.size
    tsamp, span = float(tsamp), int(span)
    if not 0 < span <= MAX_SPAN:
        raise ValueError("span must be in [1, 2^27]")
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (nchans,))
    if not np.all(np.isfinite(sigma)) or np.any(sigma < 0):
        raise ValueError("sigma must be finite and not negative")
    noise = float(np.sqrt(np.sum(sigma ** 2)))
    specs = np.zeros(len(signals), dtype=INJECT_SPEC_DTYPE)
    tmpls, amps, delays = [], [], []
    toff = 0
    for k, sig in enumerate(signals):
        sp = specs[k]
        d, _ = dispersion_delays(freqs, [sig.dm], tsamp, kdm)
        if isinstance(sig, PulsarSignal):
            if not sig.period > 2.0 * tsamp:
                raise ValueError("a period must exceed two samples")
            nbins = 1 << int(sig.log2bins) if 1 <= int(sig.log2bins) <= 16 else 0
            if not nbins:
                raise ValueError("inject: log2bins outside [1, 16]")
            kappa = np.log(2.0) / (2.0 * np.sin(np.pi * sig.ducy / 2.0) ** 2)
            phase = (np.arange(nbins, dtype=np.float64) + 0.5) / nbins
            tmpl = np.exp(kappa * (np.cos(2.0 * np.pi * phase) - 1.0))
            sp["kind"], sp["log2bins"] = 0, int(sig.log2bins)
            sp["step"] = int(round(Fraction(tsamp) / Fraction(float(sig.period)) * (1 << 64))) % (1 << 64)
            sp["phase0"] = _turns(-float(sig.phi0) % 1.0)
            sp["factor"] = accel_factor(sig.accel, tsamp)
        elif isinstance(sig, PulseSignal):
            if not sig.width > 0:
                raise ValueError("a pulse width must be positive")
            std = sig.width / tsamp / _FWHM
            half = int(np.ceil(4.0 * std))
            # arrival at the highest frequency, the reference of the delay table
            centre = (sig.time + kdm * sig.dm * freqs.max() ** -2.0) / tsamp
            mid = int(np.rint(centre))
            tmpl = np.exp(-0.5 * ((np.arange(-half, half + 1, dtype=np.float64) - (centre - mid)) / std) ** 2)
            sp["kind"], sp["length"] = 1, tmpl.size
            sp["t0"] = mid - half
            sp["factor"] = 0.0
        else:
            raise ValueError("signals must be PulsarSignal or PulseSignal")
        sp["span"] = span
        sp["tmpl_off"], sp["amp_off"], sp["delay_off"] = toff, k * nchans, k * nchans
        tmpl32 = tmpl.astype(np.float32)
        if abs(float(sp["factor"])) * span >= 1.0:
            raise ValueError("inject: |factor| * span must be below 1")
        norm = _realised_norm(sp, tmpl32, span)
        if not norm > 0.0:
            raise ValueError(f"signal {k} leaves nothing inside the {span} samples")
        w = (freqs / freqs.mean()) ** float(sig.spectral_index)
        amps.append(float(sig.snr) * noise / norm * w / w.sum())
        tmpls.append(tmpl32)
        delays.append(d[0])
        toff += tmpl32.size
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return InjectionTables(specs, cat(tmpls, np.float32), cat(amps, np.float32), cat(delays, np.int32), nchans,
                           signals, span)


def inject_host(data, tables, t_origin=0, seed=0):
    """The specification on the host (rt_inject_host, no device): a copy of
    data, uint8 / int8 / float32 [nsamp, nchans] whose row 0 is absolute sample
    t_origin, with the signals of `tables` added.  Packed rows are refused by
    their callers: an array of packed bytes is uint8 and cannot be told apart
    here."""
    out = np.array(_checked_data(data), order="C", copy=True)
    if out.shape[1] != tables.nchans:
        raise ValueError(f"the injection tables have {tables.nchans} channels, the data {out.shape[1]}")
    t_origin, seed = int(t_origin), int(seed)
    if t_origin < 0 or not 0 <= seed < 1 << 64:
        raise ValueError("inject: t_origin must not be negative and seed must be in [0, 2^64)")
    _check(_L.rt_inject_host(_lib.ptr(out), DEDISP_DTYPES[out.dtype.name], out.shape[0], out.shape[1], t_origin, seed,
                             _lib.ptr(tables.specs), tables.specs.size, _lib.ptr(tables.tmpl), tables.tmpl.size,
                             _lib.ptr(tables.amp), tables.amp.size, _lib.ptr(tables.delay), tables.delay.size))
    return out


def resolve_inject(inject, fb, nrows=None):
    """(tables, seed) of an inject= argument -- an InjectionTables or (tables,
    seed) -- checked against the file (and the rows read); None for None.
    ValueError for a packed file and for tables of another channel count."""
    if inject is None:
        return None
    tables, seed = inject if isinstance(inject, tuple) else (inject, 0)
    if not isinstance(tables, InjectionTables):
        raise ValueError("inject must be an InjectionTables or (InjectionTables, seed)")
    if _checked_sample_type(fb) is not None:
        raise ValueError("injection into packed (1-, 2-, 4- or 16-bit) files is not supported")
    if tables.nchans != fb.nchans:
        raise ValueError(f"the injection tables have {tables.nchans} channels, the file {fb.nchans}")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("inject: seed must be in [0, 2^64)")
    tables.check(np.dtype(fb.dtype).name, fb.nsamp if nrows is None else int(nrows), 0)
    return tables, seed


def _start_output(fb, out_fname):
    """Begin the injected copy of `fb`: a SIGPROC file of the source's header,
    key for key and in the source's order, and no samples yet."""
    from .reading import write_sigproc
    write_sigproc(out_fname, np.zeros((0, fb.nchans), dtype=fb.dtype), dict(fb.header))


def inject_filterbank(fb, signals_or_tables, out_fname, seed=0, sigma=None, gulp=None, device=None):
    """Write a copy of a reading.Filterbank (or a file name) with signals
    injected: the file is streamed through the device (stream_gulps), every
    gulp injected in place (engine.inject_device), downloaded and appended to
    a new SIGPROC file with the source's header.  The samples are
    inject_host's of the whole file, bit for bit, whatever the gulp.  Every
    entry point, cutouts and candidate folding included, can then run on the
    injected file unchanged.

    signals_or_tables: an InjectionTables, or signals (a list, or one) for
    injection_tables with the file's frequencies and tsamp, span = the file's
    nsamp minus the largest delay of the signals' DMs, and sigma -- None: the
    file's own rfi.channel_stats(fb).std.  Packed files are refused.  Returns
    the tables used."""
    import torch
    from . import engine
    from ._args import resolve_device
    from .dedispersion import DEFAULT_GULP_BYTES, stream_gulps
    from .reading import Filterbank, open_filterbank
    fb = fb if isinstance(fb, Filterbank) else open_filterbank(fb)
    if _checked_sample_type(fb) is not None:
        raise ValueError("injection into packed (1-, 2-, 4- or 16-bit) files is not supported")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("inject: seed must be in [0, 2^64)")
    if isinstance(signals_or_tables, InjectionTables):
        tables = signals_or_tables
    else:
        signals = signals_or_tables
        if isinstance(signals, (PulsarSignal, PulseSignal)):
            signals = [signals]
        signals = list(signals)
        _, max_delay = dispersion_delays(fb.freqs, [s.dm for s in signals] or [0.0], fb.tsamp)
        if max_delay >= fb.nsamp:
            raise ValueError(f"the largest delay ({max_delay} samples) is not below the {fb.nsamp} samples of the file")
        if sigma is None:
            from . import rfi
            sigma = rfi.channel_stats(fb, device=device).std
        tables = injection_tables(signals, fb.freqs, fb.tsamp, fb.nsamp - max_delay, sigma)
    tables, seed = resolve_inject((tables, seed), fb)
    dev = resolve_device(device)
    if gulp is None:
        gulp = max(DEFAULT_GULP_BYTES // (fb.nchans * np.dtype(fb.dtype).itemsize), 1)
    gulp = min(int(gulp), fb.nsamp)
    if gulp < 1:
        raise ValueError("gulp must be at least 1")
    _start_output(fb, out_fname)
    with torch.cuda.device(dev), open(out_fname, "ab") as f:
        def process(block, start):
            engine.inject_device(block, tables, start, seed)
            # the download waits for the kernel: the block is free again when it returns
            block.cpu().numpy().tofile(f)

        stream_gulps(fb, dev, gulp, fb.nsamp, 0, process)
    return tables
