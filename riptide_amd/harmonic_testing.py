"""Harmonic flagging and candidate filters: riptide/pipeline/harmonic_testing.py
(hdiag, htest) and the two Pipeline stages built on them,
Pipeline.flag_harmonics and Pipeline.apply_candidate_filters
(riptide/pipeline/pipeline.py:217-289).

hdiag / htest are drop-ins evaluated on the host in Python, like the
reference.  flag_harmonics tests every pair of clusters on the device
(rt_flag_harmonics: harmonic_pairs_kernel, then the rank-order resolve on the
host) and gives the result of the reference's loop; hdiag_many evaluates
hdiag's fraction and distances for many pairs in one call.
"""
import ctypes
import logging
from fractions import Fraction

import numpy as np

from . import _lib

log = logging.getLogger("riptide.pipeline")

KDM = 4.15e3   # dispersion constant of the reference, s MHz^2 cm^3 / pc

__all__ = ["hdiag", "htest", "hdiag_many", "flag_harmonics", "apply_candidate_filters"]


class _Params(ctypes.Structure):
    """rt_htest_params"""
    _fields_ = [("tobs", ctypes.c_double), ("band", ctypes.c_double), ("phase_distance_max", ctypes.c_double),
                ("dm_distance_max", ctypes.c_double), ("snr_distance_max", ctypes.c_double),
                ("denom_max", ctypes.c_uint32)]


def _band(fmin, fmax):
    return abs(fmin**-2 - fmax**-2)


def hdiag(F, H, tobs, fmin, fmax, denom_max=100):
    """Diagnostic values of the hypothesis "H is a harmonic of F".

    F, H: objects with freq (Hz), snr, ducy (width / period) and dm members.
    tobs: integration time in seconds; fmin, fmax: bottom and top observing
    frequencies; denom_max: largest denominator of the fraction fitted to
    the ratio of the two frequencies.

    Returns a dict with the reference's keys: fraction (fractions.Fraction,
    H.freq / F.freq), phase_absdiff_turns, phase_distance, dm_absdiff,
    dm_delay_absdiff, dm_distance, harmonic_snr_expected, snr_distance.
    Raises ValueError unless fmax > fmin and tobs > 0.
    """
    if not fmax > fmin:
        raise ValueError
    if not tobs > 0.0:
        raise ValueError
    # the slower one first; equal frequencies keep F first
    if H.freq < F.freq:
        slow, fast = H, F
    else:
        slow, fast = F, H
    frac = Fraction(fast.freq / slow.freq).limit_denominator(denom_max)
    turns = abs(frac * slow.freq - fast.freq) * tobs
    out = {"phase_absdiff_turns": turns, "phase_distance": turns / fast.ducy}
    if H == slow:
        frac = 1 / frac
    out["fraction"] = frac
    out["dm_absdiff"] = abs(F.dm - H.dm)
    out["dm_delay_absdiff"] = out["dm_absdiff"] * KDM * _band(fmin, fmax)
    out["dm_distance"] = out["dm_delay_absdiff"] / min(F.ducy / F.freq, H.ducy / H.freq)
    out["harmonic_snr_expected"] = F.snr / (frac.numerator * frac.denominator) ** 0.5
    out["snr_distance"] = abs(H.snr - out["harmonic_snr_expected"])
    return out


def htest(F, H, tobs, fmin, fmax, denom_max=100, phase_distance_max=1.0, dm_distance_max=3.0,
          snr_distance_max=3.0):
    """(related, fraction): whether H passes as the fraction-th harmonic of F
    -- all three of hdiag's distances within their bounds -- and the
    fraction H.freq / F.freq."""
    d = hdiag(F, H, tobs, fmin, fmax, denom_max=denom_max)
    related = (d["phase_distance"] <= phase_distance_max and d["dm_distance"] <= dm_distance_max
               and d["snr_distance"] <= snr_distance_max)
    return related, d["fraction"]


def _columns(items):
    """(freq, snr, ducy, dm) of the items as four float64 arrays."""
    return tuple(np.ascontiguousarray([getattr(x, name) for x in items], dtype=np.float64)
                 for name in ("freq", "snr", "ducy", "dm"))


def _params(tobs, fmin, fmax, denom_max, phase_distance_max=1.0, dm_distance_max=3.0, snr_distance_max=3.0):
    if int(denom_max) != denom_max or not 0 <= denom_max < 2**32:
        raise ValueError("denom_max must be an integer")
    return _Params(float(tobs), float(_band(fmin, fmax)), float(phase_distance_max), float(dm_distance_max),
                   float(snr_distance_max), int(denom_max))


def hdiag_many(F_list, H_list, tobs, fmin, fmax, denom_max=100, device=True):
    """hdiag for the pairs (F_list[k], H_list[k]) in one call: a dict of arrays
    num, den (int64; H.freq / F.freq), phase_distance, dm_distance and
    snr_distance.  device=True computes on the GPU (rt_hdiag_pairs), where
    snr_distance is within 8 * 2^-52 * max(|F.snr|, |H.snr|) of hdiag's and
    everything else identical; device=False on the host (rt_hdiag_host),
    identical to hdiag throughout.  Raises ValueError outside the engine's
    range (freq and ducy finite and positive, denom_max in [1, 1024],
    frequency ratios below 2^40)."""
    if not fmax > fmin:
        raise ValueError
    if not tobs > 0.0:
        raise ValueError
    if len(F_list) != len(H_list):
        raise ValueError("F_list and H_list differ in length")
    lib = _lib.load()
    k = len(F_list)
    cols = _columns(list(F_list) + list(H_list))
    pi = np.arange(k, dtype=np.int32)
    pj = np.arange(k, 2 * k, dtype=np.int32)
    out = {"num": np.zeros(k, np.int64), "den": np.zeros(k, np.int64), "phase_distance": np.zeros(k),
           "dm_distance": np.zeros(k), "snr_distance": np.zeros(k)}
    prm = _params(tobs, fmin, fmax, denom_max)
    fn = lib.rt_hdiag_pairs if device else lib.rt_hdiag_host
    _lib.check(fn(*(_lib.ptr(c) for c in cols), 2 * k, _lib.ptr(pi), _lib.ptr(pj), k, ctypes.addressof(prm),
                  *(_lib.ptr(out[name]) for name in ("num", "den", "phase_distance", "dm_distance",
                                                     "snr_distance"))))
    return out


def _flag_on_host(ordered, tobs, fmin, fmax, **kwargs):
    """The reference's loop: every pair in rank order, skipping a pair once
    either member is a harmonic."""
    for i, F in enumerate(ordered):
        for H in ordered[i + 1:]:
            if F.is_harmonic or H.is_harmonic:
                continue
            related, fraction = htest(F.centre, H.centre, tobs, fmin, fmax, **kwargs)
            if related:
                H.parent_fundamental = F
                H.hfrac = fraction


def _flag_on_device(ordered, tobs, fmin, fmax, block_rows=0, **kwargs):
    """rt_flag_harmonics over the clusters' centres.  False when the engine
    rejects the inputs (nothing is changed then)."""
    try:
        if not (fmax > fmin and tobs > 0.0):
            return False
        cols = _columns([c.centre for c in ordered])
        prm = _params(tobs, fmin, fmax, **kwargs)
    except (TypeError, ValueError, ArithmeticError):
        return False
    lib = _lib.load()
    n = len(ordered)
    parent = np.empty(n, np.int32)
    hnum = np.empty(n, np.int64)
    hden = np.empty(n, np.int64)
    rc = lib.rt_flag_harmonics(*(_lib.ptr(c) for c in cols), n, ctypes.addressof(prm), block_rows,
                               _lib.ptr(parent), _lib.ptr(hnum), _lib.ptr(hden))
    if rc == _lib.RT_EINVAL:
        return False
    _lib.check(rc)
    for j in np.flatnonzero(parent >= 0):
        ordered[j].parent_fundamental = ordered[parent[j]]
        ordered[j].hfrac = Fraction(int(hnum[j]), int(hden[j]))
    return True


def flag_harmonics(clusters, tobs, fmin, fmax, denom_max=100, phase_distance_max=1.0, dm_distance_max=3.0,
                   snr_distance_max=3.0):
    """Pipeline.flag_harmonics: rank the clusters by decreasing centre S/N
    (stable), then flag as a harmonic every cluster that htest relates to a
    brighter one which is not itself a harmonic, setting its
    parent_fundamental and hfrac.  Clusters already flagged stay flagged, as
    in the reference.  The pair tests run on the device; inputs outside the
    engine's range go through the host loop over htest instead, which raises
    what the reference raises."""
    if not clusters:
        log.info("No clusters found: skipping harmonic flagging")
        return
    log.info("Flagging harmonics")
    kwargs = dict(denom_max=denom_max, phase_distance_max=phase_distance_max, dm_distance_max=dm_distance_max,
                  snr_distance_max=snr_distance_max)
    ordered = sorted(clusters, key=lambda c: c.centre.snr, reverse=True)
    for rank, cl in enumerate(ordered):
        cl.rank = rank
    # the device call starts from a list without harmonics
    if any(c.is_harmonic for c in ordered) or not _flag_on_device(ordered, tobs, fmin, fmax, **kwargs):
        _flag_on_host(ordered, tobs, fmin, fmax, **kwargs)
    harmonics = sum(1 for c in clusters if c.is_harmonic)
    log.info(f"Harmonics flagged: {harmonics}")
    log.info(f"Fundamental clusters: {len(clusters) - harmonics}")
    log.info("Harmonic flagging done")


def apply_candidate_filters(clusters, params):
    """Pipeline.apply_candidate_filters: the clusters that pass, in order,
    params['dm_min'] and params['snr_min'] (None: no cut),
    params['remove_harmonics'] and params['max_number'] (None or 0: no cap;
    otherwise the brightest max_number, by decreasing S/N)."""
    log.info("Applying candidate filters")
    kept = clusters
    dm_min = params["dm_min"]
    if dm_min is not None:
        log.warning(f"Applying DM threshold of {dm_min}")
        kept = [c for c in kept if c.centre.dm >= dm_min]
    snr_min = params["snr_min"]
    if snr_min is not None:
        log.warning(f"Applying S/N threshold of {snr_min}")
        kept = [c for c in kept if c.centre.snr >= snr_min]
    if params["remove_harmonics"]:
        log.warning("Harmonic removal is enabled, clusters flagged as harmonics will NOT be output as candidates")
        kept = [c for c in kept if not c.is_harmonic]
    nmax = params["max_number"]
    if nmax:
        nleft = len(kept)
        if nleft > nmax:
            log.warning(
                f"Number of clusters remaining ({nleft}) exceeds the maximum specified number of candidates ({nmax}). "
                f"The faintest {nleft - nmax} will not be saved as candidates")
        kept = sorted(kept, key=lambda c: c.centre.snr, reverse=True)[:nmax]
    log.info(f"Candidate filters applied. Clusters remaining: {len(kept)}")
    return kept
