"""Harmonic testing on the host: rt_hdiag_host (harmonic.hpp's pair function
compiled for the CPU), the drop-ins hdiag / htest and the candidate filters,
against a restatement of riptide's rule written here with fractions.Fraction
(riptide/pipeline/harmonic_testing.py, pipeline/pipeline.py:217-289).  Every
comparison is exact: fractions as integers, distances bit for bit.

The seeded catalogue and the restatement are shared with
tests/test_gpu_harmonics.py.
"""
import functools
import itertools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

TOBS, FMIN, FMAX = 540.0, 1200.0, 1500.0
BOUNDS = dict(phase_distance_max=1.0, dm_distance_max=3.0, snr_distance_max=3.0)
PLANTED = (Fraction(2), Fraction(3), Fraction(1, 2), Fraction(3, 2), Fraction(5, 3), Fraction(7), Fraction(1, 3),
           Fraction(16))

Centre = namedtuple("Centre", "freq snr ducy dm")


# --------------------------------------------------------------------------
# the reference's rule, restated
# --------------------------------------------------------------------------
def ref_hdiag(F, H, tobs, fmin, fmax, denom_max=100):
    if not fmax > fmin or not tobs > 0.0:
        raise ValueError
    slow, fast = (H, F) if H.freq < F.freq else (F, H)      # stable: a tie keeps F first
    best = Fraction(fast.freq / slow.freq).limit_denominator(denom_max)
    turns = abs(float(best) * slow.freq - fast.freq) * tobs
    hfrac = 1 / best if H.freq < F.freq else best
    delay = abs(F.dm - H.dm) * 4.15e3 * abs(fmin ** -2 - fmax ** -2)
    expected = F.snr / float(best.numerator * best.denominator) ** 0.5
    return {
        "fraction": hfrac,
        "phase_absdiff_turns": turns,
        "phase_distance": turns / fast.ducy,
        "dm_absdiff": abs(F.dm - H.dm),
        "dm_delay_absdiff": delay,
        "dm_distance": delay / min(F.ducy / F.freq, H.ducy / H.freq),
        "harmonic_snr_expected": expected,
        "snr_distance": abs(H.snr - expected),
    }


def ref_related(d, phase_distance_max=1.0, dm_distance_max=3.0, snr_distance_max=3.0):
    return (d["phase_distance"] <= phase_distance_max and d["dm_distance"] <= dm_distance_max
            and d["snr_distance"] <= snr_distance_max)


def ref_flag(centres, tobs=TOBS, fmin=FMIN, fmax=FMAX, denom_max=100, **bounds):
    """The pipeline's loop over centres already in rank order: (parent index
    or -1, fraction or None) per centre, and the number of related pairs
    skipped because one member was already a harmonic."""
    n = len(centres)
    parent = [-1] * n
    frac = [None] * n
    skipped = 0
    for i, j in itertools.combinations(range(n), 2):
        d = ref_hdiag(centres[i], centres[j], tobs, fmin, fmax, denom_max)
        if not ref_related(d, **bounds):
            continue
        if parent[i] >= 0 or parent[j] >= 0:
            skipped += 1
            continue
        parent[j] = i
        frac[j] = d["fraction"]
    return parent, frac, skipped


# --------------------------------------------------------------------------
# the seeded catalogue
# --------------------------------------------------------------------------
def _widths():
    from riptide_amd import generate_width_trials
    return [int(w) for w in generate_width_trials(240, 0.20, 1.5)]


@functools.lru_cache(maxsize=None)
def catalogue(n=300, seed=20):
    """n centres in rank order (decreasing S/N, stable).  Periods uniform in
    0.1-10 s, S/N 7-60, ducy = ladder width / bins (240-260), DMs on a 0.1
    grid; every sixth one gets a planted harmonic (frequency jitter <= 2e-6
    relative, S/N F.snr / sqrt(pq) +- 2.5, DM +- 0.1) and that harmonic a
    harmonic of its own."""
    rng = np.random.RandomState(seed)
    widths = _widths()

    def ducy():
        return float(widths[rng.randint(len(widths))]) / float(rng.randint(240, 261))

    def harmonic_of(F, frac):
        freq = F.freq * float(frac) * (1.0 + rng.uniform(-2e-6, 2e-6))
        snr = F.snr / math.sqrt(frac.numerator * frac.denominator) + rng.uniform(-2.5, 2.5)
        dm = round(F.dm * 10 + rng.randint(-1, 2)) / 10.0
        return Centre(float(freq), float(snr), ducy(), dm)

    out = []
    k = 0
    while len(out) < n:
        c = Centre(1.0 / rng.uniform(0.1, 10.0), float(rng.uniform(7.0, 60.0)), ducy(),
                   round(rng.uniform(0.0, 100.0) * 10) / 10.0)
        out.append(c)
        if k % 6 == 0:
            h = harmonic_of(c, PLANTED[(k // 6) % len(PLANTED)])
            out.append(h)
            out.append(harmonic_of(h, PLANTED[(k // 6 + 3) % len(PLANTED)]))
        k += 1
    return tuple(sorted(out[:n], key=lambda c: c.snr, reverse=True))


@functools.lru_cache(maxsize=None)
def catalogue_table(denom_max=100):
    """ref_hdiag of every pair (i < j) of the catalogue, in combinations order."""
    cat = catalogue()
    return tuple(ref_hdiag(cat[i], cat[j], TOBS, FMIN, FMAX, denom_max)
                 for i, j in itertools.combinations(range(len(cat)), 2))


@functools.lru_cache(maxsize=None)
def catalogue_flags(denom_max=100):
    """(parent, fraction, skipped) of the catalogue from its pair table."""
    cat = catalogue()
    n = len(cat)
    parent, frac, skipped = [-1] * n, [None] * n, 0
    for (i, j), d in zip(itertools.combinations(range(n), 2), catalogue_table(denom_max)):
        if not ref_related(d, **BOUNDS):
            continue
        if parent[i] >= 0 or parent[j] >= 0:
            skipped += 1
            continue
        parent[j] = i
        frac[j] = d["fraction"]
    return tuple(parent), tuple(frac), skipped


def check_catalogue_preconditions(denom_max):
    """Conditions on the inputs, not tolerances: the catalogue exercises the
    flagging and the skip rule, and no pair sits within 1e-9 of a bound, so
    a device whose S/N distance differs in the last bits gives the same
    flags."""
    parent, _, skipped = catalogue_flags(denom_max)
    assert sum(p >= 0 for p in parent) >= 50
    assert skipped >= 50
    for d in catalogue_table(denom_max):
        for key in ("phase_distance", "dm_distance", "snr_distance"):
            assert abs(d[key] - BOUNDS[key + "_max"]) > 1e-9


EDGE_RATIOS = (1.0, 2.0, 1.5, 1.25, 2.5, 1.0 + 2.0 ** -52, float(np.nextafter(2.0, 0.0)), 99999.99999237,
               1e5 + 1.0 / 3.0, math.pi, 1.0 + 1e-9)


def edge_pairs():
    """(F, H) pairs whose frequency ratio is each edge ratio, in both orders,
    plus equal frequencies with different S/N."""
    pairs = []
    for x in EDGE_RATIOS:
        lo = Centre(0.75, 30.0, 0.02, 10.0)
        hi = Centre(0.75 * x, 12.0, 0.03, 10.1)
        if hi.freq / lo.freq != x:           # 0.75 x rounded: pick the slow frequency so the ratio is x
            lo = Centre(1.0, 30.0, 0.02, 10.0)
            hi = Centre(x, 12.0, 0.03, 10.1)
        assert hi.freq / lo.freq == x
        pairs += [(lo, hi), (hi, lo)]
    pairs.append((Centre(3.3, 25.0, 0.01, 5.0), Centre(3.3, 11.0, 0.05, 5.0)))
    pairs.append((Centre(3.3, 11.0, 0.05, 5.0), Centre(3.3, 25.0, 0.01, 5.0)))
    return pairs


def assert_same_bits(a, b, what):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    bad = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:1]}: {a[bad[:1]]} vs {b[bad[:1]]}"


def host_many(F, H, denom_max):
    from riptide_amd.harmonic_testing import hdiag_many
    return hdiag_many(F, H, TOBS, FMIN, FMAX, denom_max=denom_max, device=False)


def catalogue_pairs():
    cat = catalogue()
    idx = list(itertools.combinations(range(len(cat)), 2))
    return [cat[i] for i, _ in idx], [cat[j] for _, j in idx]


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
def test_catalogue_preconditions():
    assert len(catalogue()) == 300
    assert len(catalogue_table(100)) == 44850
    check_catalogue_preconditions(100)
    check_catalogue_preconditions(7)
    # the table-driven flags are the plain loop's
    assert ref_flag(catalogue()[:60], **BOUNDS)[0] == list(ref_flag_prefix(60))


def ref_flag_prefix(m):
    """Flags of the catalogue's first m centres from the pair table."""
    n = len(catalogue())
    parent = [-1] * m
    for (i, j), d in zip(itertools.combinations(range(n), 2), catalogue_table(100)):
        if j < m and ref_related(d, **BOUNDS) and parent[i] < 0 and parent[j] < 0:
            parent[j] = i
    return parent


@pytest.mark.parametrize("denom_max", [1, 2, 100, 1000])
def test_catalogue_fractions(denom_max):
    F, H = catalogue_pairs()
    got = host_many(F, H, denom_max)
    for k, (f, h) in enumerate(zip(F, H)):
        slow, fast = (h, f) if h.freq < f.freq else (f, h)
        want = Fraction(fast.freq / slow.freq).limit_denominator(denom_max)
        if h.freq < f.freq:
            want = 1 / want
        assert (got["num"][k], got["den"][k]) == (want.numerator, want.denominator), (k, f, h)


def test_catalogue_distances_bitwise():
    F, H = catalogue_pairs()
    got = host_many(F, H, 100)
    table = catalogue_table(100)
    for key in ("phase_distance", "dm_distance", "snr_distance"):
        assert_same_bits(got[key], [d[key] for d in table], key)
    assert [Fraction(int(a), int(b)) for a, b in zip(got["num"], got["den"])] == [d["fraction"] for d in table]
    # pow(n, 0.5) is not sqrt(n) for some of these products: the host path must be pow's
    prods = {d["fraction"].numerator * d["fraction"].denominator for d in table}
    assert any(float(p) ** 0.5 != math.sqrt(p) for p in prods)


@pytest.mark.parametrize("denom_max", [1, 2, 4, 100, 1000])
def test_edge_ratios(denom_max):
    pairs = edge_pairs()
    got = host_many([p[0] for p in pairs], [p[1] for p in pairs], denom_max)
    for k, (F, H) in enumerate(pairs):
        want = ref_hdiag(F, H, TOBS, FMIN, FMAX, denom_max)
        assert Fraction(int(got["num"][k]), int(got["den"][k])) == want["fraction"], (F, H)
        assert int(got["den"][k]) > 0 and math.gcd(int(got["num"][k]), int(got["den"][k])) == 1
        for key in ("phase_distance", "dm_distance", "snr_distance"):
            assert_same_bits([got[key][k]], [want[key]], f"{key} of {F} {H}")


def test_tie_goes_to_the_convergent():
    """Exact ties between the two bounds go to bound2, the last convergent.
    1.5 with denom_max = 1: the bounds 2/1 (semi-convergent) and 1/1
    (convergent) are both 0.5 away, and limit_denominator returns 1.  2.5 with
    denom_max = 1 ties between 3 and 2 and returns 2; 1.25 with denom_max = 2
    ties between 3/2 and 1 and returns 1."""
    for x, denom_max, want in ((1.5, 1, Fraction(1)), (2.5, 1, Fraction(2)), (1.25, 2, Fraction(1)),
                               (1.75, 2, Fraction(2)), (1.125, 4, Fraction(1))):
        assert Fraction(x).limit_denominator(denom_max) == want
        got = host_many([Centre(1.0, 20.0, 0.02, 1.0)], [Centre(x, 10.0, 0.02, 1.0)], denom_max)
        assert Fraction(int(got["num"][0]), int(got["den"][0])) == want
        got = host_many([Centre(x, 20.0, 0.02, 1.0)], [Centre(1.0, 10.0, 0.02, 1.0)], denom_max)
        assert Fraction(int(got["num"][0]), int(got["den"][0])) == 1 / want


def test_random_ratios_against_fraction():
    """Ratios log-uniform over [1, 2^39], denominators over the whole range."""
    rng = np.random.RandomState(5)
    xs = np.exp2(rng.uniform(0.0, 39.0, size=4000))
    xs[:500] = 1.0 + rng.randint(0, 1 << 20, size=500) / float(1 << 20)    # short binary expansions
    for denom_max in (1, 3, 10, 97, 1024):
        F = [Centre(1.0, 20.0, 0.02, 1.0)] * xs.size
        H = [Centre(float(x), 10.0, 0.02, 1.0) for x in xs]
        got = host_many(F, H, denom_max)
        for k, x in enumerate(xs):
            want = Fraction(float(x)).limit_denominator(denom_max)
            assert (got["num"][k], got["den"][k]) == (want.numerator, want.denominator), (x, denom_max)


def test_drop_ins_match_the_restatement():
    from riptide_amd import hdiag, htest
    cat = catalogue()
    table = catalogue_table(100)
    pairs = list(itertools.combinations(range(len(cat)), 2))
    for k in range(0, len(pairs), 37):
        i, j = pairs[k]
        got = hdiag(cat[i], cat[j], TOBS, FMIN, FMAX)
        assert set(got) == set(table[k])
        assert got["fraction"] == table[k]["fraction"] and isinstance(got["fraction"], Fraction)
        for key in table[k]:
            if key != "fraction":
                assert_same_bits([got[key]], [table[k][key]], key)
        assert htest(cat[i], cat[j], TOBS, FMIN, FMAX, **BOUNDS) == (ref_related(table[k], **BOUNDS),
                                                                      table[k]["fraction"])
    for F, H in edge_pairs():
        for denom_max in (1, 7):
            got, want = hdiag(F, H, TOBS, FMIN, FMAX, denom_max), ref_hdiag(F, H, TOBS, FMIN, FMAX, denom_max)
            assert got == want


def test_drop_ins_raise_like_the_reference():
    from riptide_amd import hdiag, htest
    from riptide_amd.harmonic_testing import hdiag_many
    F, H = Centre(1.0, 20.0, 0.02, 1.0), Centre(2.0, 10.0, 0.02, 1.0)
    for fn in (hdiag, htest, ref_hdiag):
        with pytest.raises(ValueError):
            fn(F, H, TOBS, 1500.0, 1500.0)
        with pytest.raises(ValueError):
            fn(F, H, TOBS, 1500.0, 1200.0)
        with pytest.raises(ValueError):
            fn(F, H, 0.0, FMIN, FMAX)
        with pytest.raises(ValueError):
            fn(F, H, float("nan"), FMIN, FMAX)
    with pytest.raises(ZeroDivisionError):
        hdiag(F, Centre(2.0, 10.0, 0.0, 1.0), TOBS, FMIN, FMAX)
    with pytest.raises(ValueError):
        hdiag(F, Centre(float("nan"), 10.0, 0.02, 1.0), TOBS, FMIN, FMAX)
    # the batched host call rejects what it cannot represent
    for bad in (Centre(2.0, 10.0, 0.0, 1.0), Centre(float("nan"), 10.0, 0.02, 1.0), Centre(-2.0, 10.0, 0.02, 1.0),
                Centre(2.0 ** 41, 10.0, 0.02, 1.0), Centre(2.0, 10.0, float("inf"), 1.0)):
        with pytest.raises(ValueError):
            hdiag_many([F], [bad], TOBS, FMIN, FMAX, device=False)
    for denom_max in (0, 1025):
        with pytest.raises(ValueError):
            hdiag_many([F], [H], TOBS, FMIN, FMAX, denom_max=denom_max, device=False)
    with pytest.raises(ValueError):
        hdiag_many([F], [H], 0.0, FMIN, FMAX, device=False)


class FakeCluster:
    def __init__(self, dm, snr, harmonic):
        self.centre = Centre(1.0, snr, 0.02, dm)
        self.is_harmonic = harmonic


def ref_filters(clusters, params):
    kept = list(clusters)
    if params["dm_min"] is not None:
        kept = [c for c in kept if c.centre.dm >= params["dm_min"]]
    if params["snr_min"] is not None:
        kept = [c for c in kept if c.centre.snr >= params["snr_min"]]
    if params["remove_harmonics"]:
        kept = [c for c in kept if not c.is_harmonic]
    if params["max_number"]:
        kept = sorted(kept, key=lambda c: c.centre.snr, reverse=True)[:params["max_number"]]
    return kept


@pytest.mark.parametrize("params", [
    dict(dm_min=None, snr_min=None, remove_harmonics=False, max_number=None),
    dict(dm_min=20.0, snr_min=None, remove_harmonics=False, max_number=None),
    dict(dm_min=None, snr_min=15.0, remove_harmonics=True, max_number=None),
    dict(dm_min=20.0, snr_min=9.0, remove_harmonics=True, max_number=5),
    dict(dm_min=0.0, snr_min=0.0, remove_harmonics=False, max_number=1000),
    dict(dm_min=None, snr_min=None, remove_harmonics=True, max_number=0),
    dict(dm_min=1e9, snr_min=None, remove_harmonics=False, max_number=3),
])
def test_candidate_filters(params, caplog):
    from riptide_amd import apply_candidate_filters
    rng = np.random.RandomState(11)
    clusters = [FakeCluster(float(rng.uniform(0, 60)), float(rng.choice([8.0, 12.5, 30.0, rng.uniform(7, 40)])),
                            bool(rng.randint(2))) for _ in range(40)]
    before = list(clusters)
    with caplog.at_level("INFO", logger="riptide.pipeline"):
        got = apply_candidate_filters(clusters, params)
    want = ref_filters(clusters, params)
    assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    assert clusters == before
    assert f"Candidate filters applied. Clusters remaining: {len(want)}" in caplog.text
    if params["max_number"] == 5:
        assert len(got) == 5 and "exceeds the maximum specified number of candidates (5)" in caplog.text
