"""Harmonic flagging on the device (harmonic_pairs_kernel / harmonic_diag_kernel
through rt_flag_harmonics, rt_hdiag_pairs and riptide_amd.flag_harmonics)
against the restatement of riptide's rule in tests/test_harmonics_host.py.
Fractions, flags, phase and DM distances are compared exactly; the S/N
distance, whose square root is sqrt on the device and pow on the host, within
the documented guard band 8 * 2^-52 * max(|F.snr|, |H.snr|)."""
import ctypes
import itertools
from fractions import Fraction

import numpy as np
import pytest

import test_harmonics_host as hh
from test_harmonics_host import BOUNDS, FMAX, FMIN, TOBS, Centre

pytestmark = pytest.mark.gpu

GUARD = 8 * 2.0 ** -52


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import riptide_amd
    return riptide_amd


def make_clusters(rt, centres):
    return [rt.PeakCluster([c]) for c in centres]


def c_flag(centres, block_rows=0, tobs=TOBS, denom_max=100, snr_distance_max=3.0):
    """rt_flag_harmonics on centres in rank order: (rc, parent, hnum, hden, stats)."""
    from riptide_amd import _lib
    from riptide_amd.harmonic_testing import _Params, _columns
    lib = _lib.load()
    n = len(centres)
    cols = _columns(centres) if n else tuple(np.zeros(0) for _ in range(4))
    prm = _Params(tobs, abs(FMIN ** -2 - FMAX ** -2), 1.0, 3.0, snr_distance_max, denom_max)
    parent = np.full(max(n, 1), 7, np.int32)
    hnum = np.full(max(n, 1), 7, np.int64)
    hden = np.full(max(n, 1), 7, np.int64)
    rc = lib.rt_flag_harmonics(*(_lib.ptr(c) for c in cols), n, ctypes.addressof(prm), block_rows, _lib.ptr(parent),
                               _lib.ptr(hnum), _lib.ptr(hden))
    s = [ctypes.c_uint64() for _ in range(3)]
    ms = ctypes.c_double()
    lib.rt_flag_harmonics_stats(*(ctypes.byref(x) for x in s), ctypes.byref(ms))
    stats = dict(tiles=s[0].value, near_pairs=s[1].value, host_rows=s[2].value, kernel_ms=ms.value)
    return rc, parent[:n], hnum[:n], hden[:n], stats


def assert_flags(parent, hnum, hden, want_parent, want_frac):
    assert list(parent) == list(want_parent)
    for j, f in enumerate(want_frac):
        if f is None:
            assert (hnum[j], hden[j]) == (0, 0)
        else:
            assert (hnum[j], hden[j]) == (f.numerator, f.denominator)


def test_hdiag_many_catalogue(rt):
    from riptide_amd.harmonic_testing import hdiag_many
    hh.check_catalogue_preconditions(100)
    F, H = hh.catalogue_pairs()
    assert len(F) == 44850
    dev = hdiag_many(F, H, TOBS, FMIN, FMAX, denom_max=100)
    host = hh.host_many(F, H, 100)
    assert np.array_equal(dev["num"], host["num"]) and np.array_equal(dev["den"], host["den"])
    hh.assert_same_bits(dev["phase_distance"], host["phase_distance"], "phase_distance")
    hh.assert_same_bits(dev["dm_distance"], host["dm_distance"], "dm_distance")
    band = GUARD * np.maximum(np.abs([f.snr for f in F]), np.abs([h.snr for h in H]))
    err = np.abs(dev["snr_distance"] - host["snr_distance"])
    print(f"snr_distance: max |device - host| / band = {np.max(err / band):.3f}, "
          f"{np.count_nonzero(err)} of {err.size} differ")
    assert np.all(err <= band)


@pytest.mark.parametrize("denom_max", [1, 2, 4, 100, 1000])
def test_hdiag_many_edge_ratios(rt, denom_max):
    from riptide_amd.harmonic_testing import hdiag_many
    pairs = hh.edge_pairs()
    F, H = [p[0] for p in pairs], [p[1] for p in pairs]
    dev = hdiag_many(F, H, TOBS, FMIN, FMAX, denom_max=denom_max)
    for k, (f, h) in enumerate(pairs):
        want = hh.ref_hdiag(f, h, TOBS, FMIN, FMAX, denom_max)
        assert Fraction(int(dev["num"][k]), int(dev["den"][k])) == want["fraction"], (f, h)
        hh.assert_same_bits([dev["phase_distance"][k]], [want["phase_distance"]], "phase_distance")
        hh.assert_same_bits([dev["dm_distance"][k]], [want["dm_distance"]], "dm_distance")
        assert abs(dev["snr_distance"][k] - want["snr_distance"]) <= GUARD * max(f.snr, h.snr)


@pytest.mark.parametrize("denom_max", [100, 7])
def test_flag_harmonics_catalogue(rt, denom_max):
    hh.check_catalogue_preconditions(denom_max)
    want_parent, want_frac, _ = hh.catalogue_flags(denom_max)
    cat = hh.catalogue()
    # handed over in another order: the ranks come from the stable S/N sort
    order = np.random.RandomState(3).permutation(len(cat))
    ranked = make_clusters(rt, cat)
    clusters = [ranked[k] for k in order]
    want_rank = {id(c): r for r, c in enumerate(sorted(clusters, key=lambda c: c.centre.snr, reverse=True))}
    by_rank = sorted(clusters, key=lambda c: c.centre.snr, reverse=True)
    # no two S/N are equal, so the rank order is the catalogue's
    assert all(a is b for a, b in zip(by_rank, ranked))
    rt.flag_harmonics(clusters, TOBS, FMIN, FMAX, denom_max=denom_max, **BOUNDS)
    for r, cl in enumerate(ranked):
        assert cl.rank == r == want_rank[id(cl)]
        if want_parent[r] < 0:
            assert cl.parent_fundamental is None and cl.hfrac is None and not cl.is_harmonic
        else:
            assert cl.parent_fundamental is ranked[want_parent[r]]
            assert cl.hfrac == want_frac[r] and isinstance(cl.hfrac, Fraction)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 300])
def test_flag_harmonics_shapes(rt, n):
    """Identical across tile sizes and equal to the restatement.  A prefix of
    the ranked catalogue is itself in rank order."""
    cat = hh.catalogue()[:n]
    want_parent, want_frac = (hh.catalogue_flags(100)[:2] if n == 300 else hh.ref_flag(cat, **BOUNDS)[:2])
    for block_rows in (0, 1, 64, 100):
        rc, parent, hnum, hden, stats = c_flag(cat, block_rows)
        assert rc == 0
        assert_flags(parent, hnum, hden, want_parent, want_frac)
        rows = {0: 1024}.get(block_rows, block_rows)
        assert stats["tiles"] == (0 if n <= 1 else -(-(n - 1) // rows))
        assert stats["host_rows"] == 0


def test_three_cluster_chains(rt):
    """The skip rule.  (1) B is a harmonic of A, C is related to B only: B
    is already flagged when (B, C) comes up, so C stays a fundamental.  (2) B
    and C are related to A and to each other: both get parent A."""
    A = Centre(1.0, 40.0, 0.02, 10.0)
    B = Centre(2.0, 28.0, 0.02, 10.0)             # 2nd harmonic of A: expected 40 / sqrt(2) = 28.3
    C = Centre(4.0, 19.5, 0.02, 10.0)             # 2nd harmonic of B (28 / sqrt 2 = 19.8); of A it would be 40 / 2 = 20
    cat = [A, B, C]
    want = hh.ref_flag(cat, **BOUNDS)
    assert want[0] == [-1, 0, 0] and want[2] == 1           # (B, C) related but skipped
    rc, parent, hnum, hden, _ = c_flag(cat)
    assert rc == 0
    assert_flags(parent, hnum, hden, want[0], want[1])
    assert (hnum[2], hden[2]) == (4, 1)
    # chain (1): C related to B (expected 28 / sqrt 2 = 19.8) but not to A (expected 20): S/N 16.85
    C1 = Centre(4.0, 16.85, 0.02, 10.0)
    cat = [A, B, C1]
    assert hh.ref_related(hh.ref_hdiag(B, C1, TOBS, FMIN, FMAX), **BOUNDS)
    assert not hh.ref_related(hh.ref_hdiag(A, C1, TOBS, FMIN, FMAX), **BOUNDS)
    want = hh.ref_flag(cat, **BOUNDS)
    assert want[0] == [-1, 0, -1] and want[2] == 1
    rc, parent, hnum, hden, _ = c_flag(cat)
    assert rc == 0
    assert_flags(parent, hnum, hden, want[0], want[1])
    # through the Python layer, by identity
    cl = make_clusters(rt, cat)
    rt.flag_harmonics(list(reversed(cl)), TOBS, FMIN, FMAX)
    assert [c.rank for c in cl] == [0, 1, 2]
    assert cl[1].parent_fundamental is cl[0] and cl[1].hfrac == 2 and cl[2].parent_fundamental is None


def test_near_pair_is_decided_by_the_host(rt):
    """A pair whose S/N distance is snr_distance_max to the last bit: F.snr =
    32, fraction 4 = 4/1 (pq = 4, a perfect square, so pow and sqrt both give
    2), H.snr = 32 / 2 + 3 = 19, all exact.  The device lists it as near and
    the host's verdict stands."""
    F = Centre(1.0, 32.0, 0.02, 10.0)
    H = Centre(4.0, 19.0, 0.02, 10.0)
    d = hh.ref_hdiag(F, H, TOBS, FMIN, FMAX)
    assert d["snr_distance"] == 3.0 and d["fraction"] == 4
    others = [c for c in hh.catalogue() if c.snr < 19.0][:60]
    assert len(others) == 60
    others = [c._replace(dm=c.dm + 500.0) for c in others]       # unrelated to F and H by DM
    cat = sorted([F, H] + others, key=lambda c: c.snr, reverse=True)
    want = hh.ref_flag(cat, **BOUNDS)
    assert want[0][1] == 0
    for block_rows in (0, 1):
        rc, parent, hnum, hden, stats = c_flag(cat, block_rows)
        assert rc == 0
        assert stats["near_pairs"] >= 1 and stats["host_rows"] == 0
        assert_flags(parent, hnum, hden, want[0], want[1])
    # the bound one ulp lower: the same pair is near again and now unrelated
    lower = float(np.nextafter(3.0, 0.0))
    bounds = dict(BOUNDS, snr_distance_max=lower)
    want = hh.ref_flag(cat, **bounds)
    assert want[0][1] == -1
    rc, parent, hnum, hden, stats = c_flag(cat, snr_distance_max=lower)
    assert rc == 0 and stats["near_pairs"] >= 1
    assert_flags(parent, hnum, hden, want[0], want[1])


def test_near_list_overflow_goes_to_the_host(rt):
    """100 clusters of S/N 13 and 100 of S/N 10 at one frequency: all 10 000
    bright-faint pairs sit exactly on the S/N bound, more than a tile's near
    list holds, so the tile's rows are decided on the host."""
    cat = [Centre(2.0, 13.0, 0.02, 10.0)] * 100 + [Centre(2.0, 10.0, 0.02, 10.0)] * 100
    want = hh.ref_flag(cat, **BOUNDS)
    assert sum(p >= 0 for p in want[0]) == 199      # the first claims every other one
    rc, parent, hnum, hden, stats = c_flag(cat)
    assert rc == 0
    assert stats["host_rows"] >= 1 and stats["tiles"] == 1
    assert_flags(parent, hnum, hden, want[0], want[1])
    # small tiles stay under the cap and take the near path instead
    rc, parent, hnum, hden, stats = c_flag(cat, block_rows=16)
    assert rc == 0 and stats["host_rows"] == 0 and stats["near_pairs"] > 0
    assert_flags(parent, hnum, hden, want[0], want[1])


def test_invalid_inputs(rt):
    from riptide_amd import _lib
    good = list(hh.catalogue()[:10])
    zero_ducy = good[:4] + [good[4]._replace(ducy=0.0)] + good[5:]
    nan_freq = good[:4] + [good[4]._replace(freq=float("nan"))] + good[5:]
    wide = good[:4] + [good[4]._replace(freq=good[0].freq * 2.0 ** 41)] + good[5:]
    assert c_flag(zero_ducy)[0] == _lib.RT_EINVAL
    assert c_flag(nan_freq)[0] == _lib.RT_EINVAL
    assert c_flag(wide)[0] == _lib.RT_EINVAL
    assert c_flag(good, tobs=0.0)[0] == _lib.RT_EINVAL
    assert c_flag(good, denom_max=0)[0] == _lib.RT_EINVAL
    assert c_flag(good, denom_max=1025)[0] == _lib.RT_EINVAL
    assert c_flag(good)[0] == 0

    def host_loop(centres, tobs=TOBS, fmin=FMIN, fmax=FMAX):
        for a, b in itertools.combinations(centres, 2):
            rt.htest(a, b, tobs, fmin, fmax)

    # the Python layer falls back to the host loop, which raises what the reference's loop raises
    for centres, kw in ((zero_ducy, {}), (nan_freq, {}), (good, dict(tobs=0.0)), (good, dict(fmin=1500.0))):
        with pytest.raises(Exception) as want:
            host_loop(centres, **kw)
        args = dict(dict(tobs=TOBS, fmin=FMIN, fmax=FMAX), **kw)
        with pytest.raises(type(want.value)):
            rt.flag_harmonics(make_clusters(rt, centres), args["tobs"], args["fmin"], args["fmax"])
    # outside the engine's range but fine for the reference: the fallback gives the loop's flags
    cl = make_clusters(rt, wide)
    rt.flag_harmonics(cl, TOBS, FMIN, FMAX)
    want = hh.ref_flag(wide, **BOUNDS)
    assert [(-1 if c.parent_fundamental is None else c.parent_fundamental.rank) for c in cl] == want[0]
    rt.flag_harmonics([], TOBS, FMIN, FMAX)
