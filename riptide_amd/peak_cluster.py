"""Clusters of periodogram peaks (riptide/pipeline/peak_cluster.py:4-85): the
peaks of one signal across DM trials and widths, with the rank and harmonic
relation that later pipeline stages attach.  pandas is imported only by the
two functions that return a DataFrame.
"""

_COLUMNS = ("rank", "period", "dm", "snr", "ducy", "freq", "npeaks", "hfrac_num", "hfrac_denom",
            "fundamental_rank")


class PeakCluster(list):
    """A list of Peak objects.

    rank: position in the search's S/N order (0 = brightest), or None.
    parent_fundamental: the PeakCluster this one is a harmonic of, or None for
        a fundamental.
    hfrac: fractions.Fraction, this cluster's frequency over its
        fundamental's, when there is one.
    """

    def __init__(self, peaks, rank=None, parent_fundamental=None, hfrac=None):
        super().__init__(peaks)
        self.rank = rank
        self.parent_fundamental = parent_fundamental
        self.hfrac = hfrac

    @property
    def is_harmonic(self):
        return self.parent_fundamental is not None

    @property
    def centre(self):
        """The member with the highest S/N."""
        return max(self, key=lambda p: p.snr)

    def summary_dataframe(self):
        """One row per member peak (the columns of Peak.summary_dict)."""
        import pandas
        return pandas.DataFrame.from_dict([p.summary_dict() for p in self])

    def summary_dict(self):
        """The centre's parameters plus the cluster's.  A fundamental reports
        hfrac 0/0 and its own rank as fundamental_rank, so that the columns
        stay integer in a DataFrame."""
        out = dict(self.centre.summary_dict())
        out["npeaks"] = len(self)
        out["rank"] = self.rank
        if self.is_harmonic:
            out["hfrac_num"] = self.hfrac.numerator
            out["hfrac_denom"] = self.hfrac.denominator
            out["fundamental_rank"] = self.parent_fundamental.rank
        else:
            out["hfrac_num"] = 0
            out["hfrac_denom"] = 0
            out["fundamental_rank"] = self.rank
        return out

    def __str__(self):
        return f"{type(self).__name__}(size={len(self)}, centre={self.centre})"

    __repr__ = __str__


def clusters_to_dataframe(clusters):
    """Summary of a list of PeakClusters, one row each, by decreasing S/N."""
    import pandas
    ordered = sorted(clusters, key=lambda c: c.centre.snr, reverse=True)
    return pandas.DataFrame.from_dict([c.summary_dict() for c in ordered])[list(_COLUMNS)]
