"""Refinement of a folded candidate in period and DM from its sub-band folds:
the step prepfold calls its search.  The sub-bands and the sub-integrations of
the cube Candidate.subbands are re-aligned by whole phase bins over a small
grid of DM and period offsets, and the boxcar S/N of every trial's profile is
taken (rt_refine, include/riptide_amd.h):

    y[k][s][n]    = sum over b of cube[b][s][(n + dshift[k][b]) mod N]
    prof[k][j][n] = sum over s of y[k][s][(n + pshift[j][s]) mod N]
    snr[k][j][w]  = snr1 of prof[k][j][:] at width w

The shift tables are the physics (rt_refine_shifts, double precision); the sums
are float32 in index order, the same bits on the device (refine_kernels.hip)
and in the host specification (rt_refine_host).
"""
import ctypes

import numpy as np

from . import _lib
from .dedispersion import KDM
from .ffautils import generate_width_trials

__all__ = ["Refinement", "refine_cube", "refine_candidates", "refine_shifts", "refine_host", "refine_many",
           "default_trials", "pack_refine", "REFINE_SPEC", "DEFAULT_PERIOD_STEPS", "DEFAULT_DM_STEPS"]

# rt_refine_spec (include/riptide_amd.h)
REFINE_SPEC = np.dtype([("cube_off", "<u8"), ("dshift_off", "<u8"), ("pshift_off", "<u8"), ("width_off", "<u8"),
                        ("snr_off", "<u8"), ("prof_off", "<u8"), ("bands", "<u4"), ("subints", "<u4"),
                        ("bins", "<u4"), ("ndm", "<u4"), ("nper", "<u4"), ("nw", "<u4"), ("stdnoise", "<f4"),
                        ("reserved", "<u4")], align=True)

# Half-widths of the default trial grids, in steps of one phase bin: interface
# defaults, not tuned values.
DEFAULT_PERIOD_STEPS = 16
DEFAULT_DM_STEPS = 32


class Refinement:
    """What refine_cube found.

    periods [J], dms [K], widths [W]: the trials.
    snr [K, J, W] float32; snr_map [K, J]: its maximum over the widths.
    best_period, best_dm, best_width, best_snr: the trial of the largest S/N
        (a tie goes to the lowest flat index of snr).
    profile [N] float32: the best trial's profile.
    """

    def __init__(self, periods, dms, widths, snr, profile=None):
        self.periods = np.asarray(periods, dtype=np.float64)
        self.dms = np.asarray(dms, dtype=np.float64)
        self.widths = np.asarray(widths, dtype=np.uint32)
        self.snr = np.asarray(snr, dtype=np.float32)
        if self.snr.shape != (self.dms.size, self.periods.size, self.widths.size):
            raise ValueError("snr must be [dms, periods, widths]")
        self.snr_map = self.snr.max(axis=2)
        k, j, w = np.unravel_index(int(np.argmax(self.snr)), self.snr.shape)
        self.best_index = (int(k), int(j), int(w))
        self.best_dm = float(self.dms[k])
        self.best_period = float(self.periods[j])
        self.best_width = int(self.widths[w])
        self.best_snr = float(self.snr[k, j, w])
        self.profile = profile

    def __repr__(self):
        return (f"Refinement(best_period={self.best_period!r}, best_dm={self.best_dm!r}, "
                f"best_width={self.best_width}, best_snr={self.best_snr:.3f})")


def refine_shifts(period, tobs, bins, subints, band_freqs, dm, periods, dms, kdm=KDM):
    """(pshift int32 [J, S], dshift int32 [K, B]), entries in [0, bins): the
    whole-bin rotations that re-align the sub-integrations of a fold at
    `period` spanning `tobs` seconds to each trial period, and its sub-bands
    (centre frequencies `band_freqs`, MHz) folded at `dm` to each trial DM
    (rt_refine_shifts; host only)."""
    f = np.ascontiguousarray(np.atleast_1d(band_freqs), dtype=np.float64)
    periods = np.ascontiguousarray(np.atleast_1d(periods), dtype=np.float64)
    dms = np.ascontiguousarray(np.atleast_1d(dms), dtype=np.float64)
    if f.ndim != 1 or periods.ndim != 1 or dms.ndim != 1:
        raise ValueError("band_freqs, periods and dms must be one-dimensional")
    bins, subints = int(bins), int(subints)
    if bins < 0 or subints < 0:
        raise ValueError("refine: bins and subints must not be negative")
    pshift = np.zeros((periods.size, subints), dtype=np.int32)
    dshift = np.zeros((dms.size, f.size), dtype=np.int32)
    L = _lib.load()
    _lib.check(L.rt_refine_shifts(float(period), float(tobs), bins, subints, _lib.ptr(f), f.size, float(dm),
                                  float(kdm), _lib.ptr(periods), periods.size, _lib.ptr(dms), dms.size,
                                  _lib.ptr(pshift), _lib.ptr(dshift)))
    return pshift, dshift


def _as_cube(cube):
    x = np.ascontiguousarray(cube, dtype=np.float32)
    if x.ndim == 2:
        x = x[:, None, :]
    if x.ndim != 3:
        raise ValueError("cube must be [bands, subints, bins] or [bands, bins]")
    return x


def _as_job(cube, dshift, pshift, widths, stdnoise):
    x = _as_cube(cube)
    B, S, _ = x.shape
    d = np.ascontiguousarray(dshift, dtype=np.int32)
    p = np.ascontiguousarray(pshift, dtype=np.int32)
    if d.ndim != 2 or d.shape[1] != B or p.ndim != 2 or p.shape[1] != S:
        raise ValueError("dshift must be [K, bands] and pshift [J, subints]")
    w = np.ascontiguousarray(np.atleast_1d(widths))
    if w.ndim != 1 or (w.size and (w.min() < 0 or w.max() > 0xFFFFFFFF)):
        raise ValueError("trial widths must be all > 0 and < columns")
    return x, d, p, w.astype(np.uint32), float(stdnoise)


def refine_host(cube, dshift, pshift, widths, stdnoise, profiles=False):
    """The host specification (rt_refine_host, sequential, no device): snr
    float32 [K, J, W], and with profiles=True also prof [K, J, N]."""
    x, d, p, w, stdnoise = _as_job(cube, dshift, pshift, widths, stdnoise)
    B, S, N = x.shape
    K, J = d.shape[0], p.shape[0]
    snr = np.zeros((K, J, w.size), dtype=np.float32)
    prof = np.zeros((K, J, N), dtype=np.float32) if profiles else None
    L = _lib.load()
    _lib.check(L.rt_refine_host(_lib.ptr(x), B, S, N, _lib.ptr(d), K, _lib.ptr(p), J, _lib.ptr(w), w.size, stdnoise,
                                _lib.ptr(snr), _lib.ptr(prof) if profiles else None))
    return (snr, prof) if profiles else snr


def pack_refine(jobs):
    """The packed arrays of one batched call for `jobs`, a list of (cube,
    dshift, pshift, widths, stdnoise): (cubes float32, shifts int32, widths
    uint32, table of REFINE_SPEC, shapes [(K, J, W, N)], S/N floats, profile
    floats), every candidate's arrays back to back."""
    table = np.zeros(len(jobs), dtype=REFINE_SPEC)
    cubes, shifts, widths, shapes = [], [], [], []
    co = so = wo = no = po = 0
    for i, job in enumerate(jobs):
        x, d, p, w, stdnoise = _as_job(*job)
        B, S, N = x.shape
        K, J, W = d.shape[0], p.shape[0], w.size
        table[i] = (co, so, so + d.size, wo, no, po, B, S, N, K, J, W, stdnoise, 0)
        cubes.append(x.ravel())
        shifts += [d.ravel(), p.ravel()]
        widths.append(w)
        shapes.append((K, J, W, N))
        co += x.size
        so += d.size + p.size
        wo += W
        no += K * J * W
        po += K * J * N
    cat = (lambda parts, dt: np.ascontiguousarray(np.concatenate(parts), dtype=dt) if parts else np.zeros(0, dt))
    return cat(cubes, np.float32), cat(shifts, np.int32), cat(widths, np.uint32), table, shapes, no, po


def refine_many(jobs, profiles=False):
    """One device call (rt_refine) for `jobs`, a list of (cube, dshift,
    pshift, widths, stdnoise) of any shapes (bins <= 1024): a list of snr
    [K, J, W], or of (snr, prof [K, J, N]) with profiles=True.  The tables are
    validated as refine_host validates them."""
    jobs = list(jobs)
    if not jobs:
        return []
    cubes, shifts, widths, table, shapes, nsnr, nprof = pack_refine(jobs)
    snr = np.zeros(nsnr, dtype=np.float32)
    prof = np.zeros(nprof, dtype=np.float32) if profiles else None
    L = _lib.load()
    _lib.check(L.rt_refine(_lib.ptr(cubes), _lib.ptr(shifts), _lib.ptr(widths), _lib.ptr(table), len(jobs),
                           _lib.ptr(snr), _lib.ptr(prof) if profiles else None))
    out = []
    for i, (K, J, W, N) in enumerate(shapes):
        o = int(table["snr_off"][i])
        s = snr[o:o + K * J * W].reshape(K, J, W).copy()
        if profiles:
            o = int(table["prof_off"][i])
            out.append((s, prof[o:o + K * J * N].reshape(K, J, N).copy()))
        else:
            out.append(s)
    return out


def default_trials(period, tobs, bins, band_freqs, dm, kdm=KDM):
    """(periods, dms) of the default grid: periods 1 / (1 / P - j / (N *
    tobs)) for j = -16..16, one bin of drift over the span per step, and DMs
    dm + k * P / (N * kdm * (fmin^-2 - fmax^-2)) for k = -32..32, one bin of
    delay at the lowest band per step, those below zero dropped (a single band
    has no DM axis: the fold's DM alone).  The counts (DEFAULT_PERIOD_STEPS,
    DEFAULT_DM_STEPS) are interface defaults, not tuned values."""
    period, tobs, bins = float(period), float(tobs), int(bins)
    f = np.atleast_1d(np.asarray(band_freqs, dtype=np.float64))
    j = np.arange(-DEFAULT_PERIOD_STEPS, DEFAULT_PERIOD_STEPS + 1, dtype=np.float64)
    periods = 1.0 / (1.0 / period - j / (bins * tobs))
    span = f.min() ** -2.0 - f.max() ** -2.0
    if span > 0:
        k = np.arange(-DEFAULT_DM_STEPS, DEFAULT_DM_STEPS + 1, dtype=np.float64)
        dms = float(dm) + k * period / (bins * float(kdm) * span)
        dms = dms[dms >= 0]
    else:
        dms = np.array([float(dm)])
    return periods, dms


def _default_stdnoise(x):
    """sqrt(bands that are not all zero): every band series was normalised on
    its own, so a bin of a band's fold has unit variance and the bands add."""
    live = int(np.count_nonzero(np.any(x.reshape(x.shape[0], -1) != 0, axis=1)))
    return float(np.sqrt(max(live, 1)))


def _best_profile(x, dshift, pshift):
    """The profile of one trial by the specification's ordered float32 sums."""
    B, S, N = x.shape
    y = np.zeros((S, N), dtype=np.float32)
    for b in range(B):
        y = y + np.roll(x[b], -int(dshift[b]), axis=1)
    p = np.zeros(N, dtype=np.float32)
    for s in range(S):
        p = p + np.roll(y[s], -int(pshift[s]))
    return p


def _job(cube, band_freqs, period, tobs, dm, periods, dms, widths, stdnoise, kdm):
    x = _as_cube(cube)
    B, S, N = x.shape
    dp, dd = default_trials(period, tobs, N, band_freqs, dm, kdm)
    periods = dp if periods is None else np.atleast_1d(np.asarray(periods, dtype=np.float64))
    dms = dd if dms is None else np.atleast_1d(np.asarray(dms, dtype=np.float64))
    widths = generate_width_trials(N) if widths is None else np.atleast_1d(widths)
    stdnoise = _default_stdnoise(x) if stdnoise is None else float(stdnoise)
    pshift, dshift = refine_shifts(period, tobs, N, S, band_freqs, dm, periods, dms, kdm)
    return (x, dshift, pshift, widths, stdnoise), periods, dms


def _finish(job, periods, dms, snr):
    x, dshift, pshift, widths, _ = job
    r = Refinement(periods, dms, widths, snr)
    k, j, _ = r.best_index
    r.profile = _best_profile(x, dshift[k], pshift[j])
    return r


def refine_cube(cube, band_freqs, period, tobs, dm, periods=None, dms=None, widths=None, stdnoise=None, kdm=KDM,
                device=True):
    """Refine one folded cube [bands, subints, bins] (or [bands, bins]: one
    sub-integration), folded at `period` seconds and `dm` over `tobs` seconds
    of whole periods, with band centre frequencies `band_freqs` in MHz: a
    Refinement.

    Defaults: widths generate_width_trials(bins); stdnoise sqrt(bands that are
    not all zero); periods and dms the grid of default_trials, 33 period and
    up to 65 DM trials one phase bin apart.  Those counts are interface
    defaults, not tuned values: pass periods / dms for any other grid.
    device=False runs the host specification (rt_refine_host) instead of the
    kernels; the profiles of the two have the same bits."""
    job, periods, dms = _job(cube, band_freqs, period, tobs, dm, periods, dms, widths, stdnoise, kdm)
    snr = refine_many([job])[0] if device else refine_host(*job)
    return _finish(job, periods, dms, snr)


def candidate_tobs(cand, nsamp=None):
    """The span in seconds of a Candidate's fold: m * period, m the whole
    periods rt_fold_shape gives for the series length of its tsmeta (tobs /
    tsamp samples, or `nsamp` when the folded series was shorter)."""
    period, tsamp = float(cand.params["period"]), float(cand.tsmeta["tsamp"])
    bins = int(cand.subbands.shape[-1])
    nsamp = int(round(float(cand.tsmeta["tobs"]) / tsamp)) if nsamp is None else int(nsamp)
    m = ctypes.c_size_t()
    L = _lib.load()
    _lib.check(L.rt_fold_shape(nsamp, period / bins / tsamp, bins, 0, ctypes.byref(m), None))
    return m.value * period


def refine_candidates(cands, periods=None, dms=None, widths=None, stdnoise=None, kdm=KDM, device=True, nsamp=None):
    """refine_cube for every Candidate of `cands` that has `subbands`, all in
    one device call (rt_refine): sets each one's `refined` (a Refinement; the
    others keep None) and returns `cands`.  periods / dms / widths / stdnoise:
    None for each candidate's defaults, or one value for all."""
    todo = [c for c in cands if getattr(c, "subbands", None) is not None]
    jobs = []
    for c in todo:
        jobs.append(_job(c.subbands, c.band_freqs, c.params["period"], candidate_tobs(c, nsamp), c.tsmeta["dm"],
                         periods, dms, widths, stdnoise, kdm))
    snrs = refine_many([j[0] for j in jobs]) if device else [refine_host(*j[0]) for j in jobs]
    for c, (job, per, dm), snr in zip(todo, jobs, snrs):
        c.refined = _finish(job, per, dm, snr)
    return cands
