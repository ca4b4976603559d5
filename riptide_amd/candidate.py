"""Candidates: the pipeline's final product (riptide/candidate.py:14-146) and
the stage that builds them from peak clusters (pipeline/pipeline.py:86-133,
292-333).  Each DM trial is loaded, dereddened and normalised once, and all
of its clusters are folded by one batched device call (folding.fold_many).
Plotting is not part of this module.
"""
import logging
import traceback
from collections import defaultdict

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
    """

    def __init__(self, params, tsmeta, peaks, subints):
        self.params = params
        self.tsmeta = tsmeta
        self.peaks = peaks
        self.subints = subints

    @property
    def profile(self):
        """Folded profile, one value per phase bin."""
        return self.subints if self.subints.ndim == 1 else self.subints.sum(axis=0)

    @property
    def dm_curve(self):
        """(dm trials, best S/N across widths at each)."""
        best = self.peaks.copy().groupby("dm").max()
        return best.index.values, best.snr.values

    def to_dict(self):
        return {"params": self.params, "tsmeta": self.tsmeta, "peaks": self.peaks, "subints": self.subints}

    @classmethod
    def from_dict(cls, items):
        return cls(items["params"], items["tsmeta"], items["peaks"], items["subints"])

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
