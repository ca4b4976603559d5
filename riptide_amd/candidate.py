"""Candidates: the pipeline's final product (riptide/candidate.py:14-146) and
the stage that builds them from peak clusters (pipeline/pipeline.py:86-133,
292-333).  Each DM trial is loaded, dereddened and normalised once, and all
of its clusters are folded by one batched device call (folding.fold_many).
build_candidates_filterbank starts from the channelised file instead: it
dedisperses, normalises and folds on the device, and its candidates also carry
the fold of every sub-band, the frequency-phase diagnostic.
Plotting is not part of this module.
"""
import logging
import traceback
from collections import defaultdict, namedtuple

import numpy as np

from .folding import check_fold_args, fold_many, fold_shape

log = logging.getLogger("riptide.candidate")


def effective_subints(ts_length, period, subints):
    """The sub-integrations actually asked of fold(): None (one per whole
    period) when `subints` periods do not fit in the data (candidate.py:89-95)."""
    if subints is not None and subints * period >= ts_length:
        log.debug(f"Period ({period:.3f}) x requested subints ({subints:d}) exceeds time series length "
                  f"({ts_length:.3f}), setting subints = full periods that fit in the data")
        return None
    return subints


class Candidate:
    """A folded candidate.

    params: best-fit parameters of the signal: period, freq, dm, width, ducy,
        snr (the centre peak's summary_dict).
    tsmeta: Metadata of the DM trial it was folded from.
    peaks: pandas.DataFrame of the member peaks of its cluster.
    subints: folded sub-integrations, (num_subints, num_bins), or (num_bins,)
        for a single one.
    subbands: None, or the same fold of every sub-band of the channelised
        data, float32 (num_bands, num_subints, num_bins), or (num_bands,
        num_bins) for a single sub-integration (build_candidates_filterbank).
    band_freqs: None, or the mean channel frequency of each sub-band in MHz.
    refined: None, or the refine.Refinement of `subbands` over period and DM
        offsets (refine.refine_candidates); `params` is not altered by it.
    """

    def __init__(self, params, tsmeta, peaks, subints, subbands=None, band_freqs=None, refined=None):
        self.params = params
        self.tsmeta = tsmeta
        self.peaks = peaks
        self.subints = subints
        self.subbands = subbands
        self.band_freqs = band_freqs
        self.refined = refined

    @property
    def profile(self):
        """Folded profile, one value per phase bin."""
        return self.subints if self.subints.ndim == 1 else self.subints.sum(axis=0)

    @property
    def dm_curve(self):
        """(dm trials, best S/N across widths at each)."""
        best = self.peaks.copy().groupby("dm").max()
        return best.index.values, best.snr.values

    @property
    def freq_phase(self):
        """Frequency against phase, (num_bands, num_bins): every sub-band's
        folded profile.  None without sub-bands."""
        if self.subbands is None:
            return None
        return self.subbands if self.subbands.ndim == 2 else self.subbands.sum(axis=1)

    def to_dict(self):
        items = {"params": self.params, "tsmeta": self.tsmeta, "peaks": self.peaks, "subints": self.subints}
        if self.subbands is not None:
            items["subbands"] = self.subbands
        if self.band_freqs is not None:
            items["band_freqs"] = self.band_freqs
        if self.refined is not None:
            items["refined"] = self.refined
        return items

    @classmethod
    def from_dict(cls, items):
        return cls(items["params"], items["tsmeta"], items["peaks"], items["subints"],
                   subbands=items.get("subbands"), band_freqs=items.get("band_freqs"),
                   refined=items.get("refined"))

    @classmethod
    def from_folded(cls, ts, peak_cluster, subints_array):
        """params are the centre peak's (period, freq, dm, width, ducy, snr),
        as in candidate.py:98."""
        return cls(peak_cluster.centre.summary_dict(), ts.metadata, peak_cluster.summary_dataframe(),
                   subints_array)

    @classmethod
    def from_pipeline_output(cls, ts, peak_cluster, bins, subints=1):
        """Fold `ts` at the cluster centre's period.  `subints` may be None
        (one per whole period), which is also what is used when `subints`
        periods do not fit in the data."""
        period = peak_cluster.centre.period
        subints = effective_subints(ts.length, period, subints)
        return cls.from_folded(ts, peak_cluster, ts.fold(period, bins, subints=subints))

    def __str__(self):
        return f"{type(self).__name__}({self.params})"

    __repr__ = __str__


def get_search_range(range_confs, period):
    """The search range configuration (a copy) that `period` falls into:
    ranges ordered by period_max; a period below every range gets the first
    (with a warning), one at or above every range the last."""
    ranges = sorted(range_confs, key=lambda r: r["ffa_search"]["period_max"])
    pmin_global = min(r["ffa_search"]["period_min"] for r in ranges)
    pmax_global = max(r["ffa_search"]["period_max"] for r in ranges)
    if period < pmin_global:
        log.warning(f"Given period={period:.9f} is shorter than the minimum search period={pmin_global:.9f}."
                    " This will not affect the processing but it should NOT be happening.")
        return dict(ranges[0])
    if period >= pmax_global:      # the search runs slightly past period_max
        return dict(ranges[-1])
    for r in ranges:
        if r["ffa_search"]["period_min"] <= period < r["ffa_search"]["period_max"]:
            return dict(r)
    return None


def candidate_fold_spec(ts, cluster, range_confs):
    """(period, bins, subints) that fold_many is asked for `cluster`: the
    bins / subints of its period's range, subints turned into None when they
    do not fit.  Raises what folding the candidate would raise (fold()'s
    argument errors, or no whole period fitting in the data), so that
    build_candidates can leave the cluster out before the batched call."""
    period = cluster.centre.period
    conf = get_search_range(range_confs, period)["candidates"]
    bins = int(conf["bins"])
    subints = effective_subints(ts.length, period, conf["subints"])
    factor, subints = check_fold_args(ts.length, ts.tsamp, period, bins, subints)
    if bins != 1:
        fold_shape(ts.nsamp, factor, bins, subints)
    return period, bins, subints


def build_candidates(clusters, load_series, range_confs, deredden_params):
    """Candidates of a list of PeakClusters, by decreasing S/N.

    load_series(dm) returns the TimeSeries of a DM trial and is called once
    per distinct centre DM; the series is dereddened (deredden_params:
    rmed_width, rmed_minpts) and normalised, and every cluster of that DM is
    folded with the bins / subints of its period's range
    (range_confs[k]["candidates"]).  A cluster that cannot be folded is logged
    and left out."""
    ordered = sorted(clusters, key=lambda c: c.centre.snr, reverse=True)
    if not ordered:
        log.info("No clusters: no candidates to build")
        return []
    by_dm = defaultdict(list)
    for cl in ordered:
        by_dm[cl.centre.dm].append(cl)
    log.debug(f"{len(ordered)} candidates to build from {len(by_dm)} TimeSeries")

    candidates = []
    for dm, group in by_dm.items():
        ts = load_series(dm).deredden(deredden_params["rmed_width"], minpts=deredden_params["rmed_minpts"])
        ts = ts.normalise()
        todo, specs = [], []
        for cl in group:
            try:
                specs.append(candidate_fold_spec(ts, cl, range_confs))
                todo.append(cl)
            except Exception as err:
                log.error(err)
                log.error(traceback.format_exc())
        for cl, arr in zip(todo, fold_many(ts, specs)):
            candidates.append(Candidate.from_folded(ts, cl, arr))
    candidates.sort(key=lambda c: c.params["snr"], reverse=True)
    log.info(f"Total candidates: {len(candidates)}")
    return candidates


class _SeriesShape(namedtuple("_SeriesShape", "nsamp tsamp")):
    """What candidate_fold_spec asks of a TimeSeries, for series that stay on
    the device."""

    @property
    def length(self):
        return self.nsamp * self.tsamp


def build_candidates_filterbank(clusters, fb_or_fname, range_confs, deredden_params, nsub=32, mask=None,
                                zero_dm=False, kdm=None, nout=None, budget_bytes=None, device=None, refine=False,
                                block_mask=None):
    """Candidates of a list of PeakClusters, by decreasing S/N, straight from
    the channelised file (a name for reading.open_filterbank, or a Filterbank /
    PackedFilterbank): build_candidates without a load_series, and every
    Candidate also carries `subbands`, the fold of each of `nsub` contiguous
    sub-bands (dedispersion.band_edges), and `band_freqs`.

    The distinct centre DMs are taken in batches sized by budget_bytes (default:
    dedispersion.DEFAULT_BUDGET_BYTES; the band series and their normalised copy
    are counted).  A batch is one pass over the file: dedispersion.band_series
    gives every DM's nsub sub-bands and, as the last band, the full band,
    dereddened (deredden_params: rmed_width, rmed_minpts) and normalised; one
    engine.fold_device call then folds every (cluster, band) with the bins /
    subints of the cluster's period range.  `subints` is the full-band fold,
    what build_candidates gives for the same series; a sub-band with no
    unmasked channel folds to zeros.

    nout: samples of every series (default: nsamp minus the largest delay over
    those DMs; pass the search's own nout to fold exactly what was searched).
    mask, zero_dm, kdm, block_mask: as for search_filterbank.  tsmeta is the file's
    metadata with `dm` set, as search_filterbank's trials have it.  A cluster
    that cannot be folded is logged and left out.

    refine=True: every candidate is then refined in period and DM from its
    sub-bands (refine.refine_candidates with its defaults, one device call) and
    carries the result as `refined`."""
    import torch
    from . import engine
    from .dedispersion import DEFAULT_BUDGET_BYTES, KDM, band_edges, band_series, check_max_delay, dispersion_delays
    from .reading import Filterbank, open_filterbank
    fb = fb_or_fname if isinstance(fb_or_fname, Filterbank) else open_filterbank(fb_or_fname)
    kdm = KDM if kdm is None else float(kdm)
    budget_bytes = DEFAULT_BUDGET_BYTES if budget_bytes is None else int(budget_bytes)
    ordered = sorted(clusters, key=lambda c: c.centre.snr, reverse=True)
    if not ordered:
        log.info("No clusters: no candidates to build")
        return []
    by_dm = defaultdict(list)
    for cl in ordered:
        by_dm[float(cl.centre.dm)].append(cl)
    dms = list(by_dm)
    log.debug(f"{len(ordered)} candidates to build from {len(dms)} DMs of {fb.header.fname}")
    _, max_delay = dispersion_delays(fb.freqs, dms, fb.tsamp, kdm)
    check_max_delay(max_delay, fb.nsamp)
    nout = fb.nsamp - max_delay if nout is None else int(nout)
    bands = np.concatenate([band_edges(fb.nchans, nsub), np.array([[0, fb.nchans]], dtype=np.uint32)])
    nbands = bands.shape[0]
    band_freqs = np.array([fb.freqs[lo:hi].mean() for lo, hi in bands[:nsub]])
    shape = _SeriesShape(nout, fb.tsamp)
    # the raw band series of a DM and their normalised copy, half the budget: the
    # rest is left to the gulp buffers and the dereddening workspace
    per_dm = 2 * nbands * nout * 4
    batch = max(1, int(budget_bytes // 2 // per_dm))

    candidates = []
    for b0 in range(0, len(dms), batch):
        group = dms[b0:b0 + batch]
        series, _ = band_series(fb, group, bands, deredden_params, nout, mask=mask, zero_dm=zero_dm, kdm=kdm,
                                device=device, budget_bytes=budget_bytes, block_mask=block_mask)
        todo, specs = [], []
        for i, dm in enumerate(group):
            for cl in by_dm[dm]:
                try:
                    period, bins, subints = candidate_fold_spec(shape, cl, range_confs)
                    if bins < 2:
                        raise ValueError("the device fold needs bins >= 2")
                except Exception as err:
                    log.error(err)
                    log.error(traceback.format_exc())
                    continue
                todo.append((cl, dm))
                specs += [(i * nbands + b, period, bins, subints) for b in range(nbands)]
        folds = engine.fold_device(series.view(len(group) * nbands, nout), fb.tsamp, specs)
        for k, (cl, dm) in enumerate(todo):
            # a cluster's band folds have one shape: one download
            arrs = torch.stack(folds[k * nbands:(k + 1) * nbands]).cpu().numpy()
            candidates.append(Candidate(cl.centre.summary_dict(), fb.metadata(dm), cl.summary_dataframe(),
                                        arrs[-1].copy(), subbands=arrs[:-1].copy(), band_freqs=band_freqs))
    if refine:
        from .refine import refine_candidates
        refine_candidates(candidates, kdm=kdm, nsamp=nout)
    candidates.sort(key=lambda c: c.params["snr"], reverse=True)
    log.info(f"Total candidates: {len(candidates)}")
    return candidates
