"""CPU-only tests of the candidate refinement's host layer: the shift tables
(rt_refine_shifts) against a numpy float64 restatement, the specification
(rt_refine_host) against a numpy roll-and-sum and the oracle's S/N, recovery
of an off-centre trial, the Python layer and the sanitizer program.  No call
reaches the GPU."""
import os
import subprocess

import numpy as np
import pytest

import refine_common as rc
from conftest import REPO, snr_close

FREQS7 = np.array([1510.0, 1497.5, 1440.0, 1433.0, 1391.0, 1302.0, 1288.5])   # unevenly spaced, unsorted below


@pytest.mark.parametrize("N", [2, 3, 64, 257, 1024])
@pytest.mark.parametrize("S", [1, 2, 33])
def test_shift_tables(N, S):
    from riptide_amd.refine import refine_shifts
    P, T, dm, kdm = 0.7130001, 431.0 * 0.7130001, 42.0, rc.KDM
    f = FREQS7[[3, 0, 6, 1, 5, 2, 4]]
    j = np.array([-7.0, -2.5, -1.0, 0.0, 1.0, 3.25, 5.0 * N])       # the last one wraps the outer subints
    periods = 1.0 / (1.0 / P - j / (N * T))
    span = f.min() ** -2.0 - f.max() ** -2.0
    step = P / (N * kdm * span)
    # both sides of the centre, the centre itself, and offsets that wrap the
    # lowest band more than once (2.5 and 9 turns)
    dms = dm + step * np.array([-9.0 * N, -3.0, -0.5, 0.0, 1.0, 2.0, 2.5 * N + 0.25])
    pshift, dshift = refine_shifts(P, T, N, S, f, dm, periods, dms, kdm)
    ps, ds, vp, vd = rc.numpy_shifts(P, T, N, S, f, dm, kdm, periods, dms)
    assert pshift.dtype == np.int32 and pshift.shape == (7, S) and dshift.shape == (7, 7)
    assert np.array_equal(pshift, ps) and np.array_equal(dshift, ds)
    assert pshift.min() >= 0 and pshift.max() < N and dshift.min() >= 0 and dshift.max() < N
    assert not pshift[3].any() and not dshift[3].any()            # the centre trial
    assert np.abs(vd[-1]).max() > 2 * N and np.abs(vd[0]).max() > 2 * N       # wrapped more than once
    if S > 1:
        assert np.abs(vp).max() >= N
    # the band at fmax never moves
    assert not dshift[:, 1].any()


def test_shift_table_errors():
    from riptide_amd.refine import refine_shifts
    f, per, dms = [1400.0, 1300.0], [0.5, 0.5001], [10.0, 11.0]
    refine_shifts(0.5, 100.0, 16, 3, f, 10.0, per, dms)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="fold period"):
            refine_shifts(bad, 100.0, 16, 3, f, 10.0, per, dms)
        with pytest.raises(ValueError, match="fold span"):
            refine_shifts(0.5, bad, 16, 3, f, 10.0, per, dms)
        with pytest.raises(ValueError, match="trial periods"):
            refine_shifts(0.5, 100.0, 16, 3, f, 10.0, [0.5, bad], dms)
        with pytest.raises(ValueError, match="band frequencies"):
            refine_shifts(0.5, 100.0, 16, 3, [bad, 1300.0], 10.0, per, dms)
    with pytest.raises(ValueError, match="bins must be >= 2"):
        refine_shifts(0.5, 100.0, 1, 3, f, 10.0, per, dms)
    for kw in ({"subints": 0}, {"f": []}, {"per": []}, {"dms": []}):
        with pytest.raises(ValueError, match="must be >= 1"):
            refine_shifts(0.5, 100.0, 16, kw.get("subints", 3), kw.get("f", f), 10.0, kw.get("per", per),
                          kw.get("dms", dms))
    with pytest.raises(ValueError, match="DM shift of 2\\^31"):
        refine_shifts(0.5, 100.0, 16, 3, f, 10.0, per, [10.0, 1e30])
    with pytest.raises(ValueError, match="DM shift of 2\\^31"):
        refine_shifts(0.5, 100.0, 16, 3, f, 10.0, per, [10.0, np.nan])
    with pytest.raises(ValueError, match="period shift of 2\\^31"):
        refine_shifts(0.5, 1e6, 16, 3, f, 10.0, [0.5, 1e-12], dms)


# the last three: three chunks of band and of sub-integration rows (the device
# loads 256 rows of shifts at a time), and three bins per device thread
HOST_SHAPES = [(1, 1, 2), (2, 1, 3), (7, 2, 65), (3, 33, 64), (513, 2, 31), (2, 513, 16), (3, 2, 700)]


@pytest.mark.parametrize("B,S,N", HOST_SHAPES)
def test_host_against_numpy(oracle, B, S, N):
    from riptide_amd.refine import refine_host
    rng = np.random.RandomState(B * 1000 + S * 10 + N)
    d, p = rc.tables(rng, B, S, N, 3, 3)
    assert d.min() == 0 and d.max() == N - 1 and p.min() == 0 and p.max() == N - 1
    for t in (d, p):
        if t.shape[1] > rc.CHUNK:
            rc.check_chunked_table(t, N)
    w = rc.widths_for(N)
    assert w[0] == 1 and w[-1] == N - 1
    stdnoise = 1.7
    # small integers: every partial sum is exact in float32
    x = rc.cube(rng, B, S, N, "int")
    snr, prof = refine_host(x, d, p, w, stdnoise, profiles=True)
    ref, _ = rc.numpy_profiles(x, d, p)
    assert prof.dtype == np.float32 and np.array_equal(prof.astype(np.float64), ref)
    ok, msg = snr_close(snr.reshape(-1, w.size), oracle.snr2(prof.reshape(-1, N), w, stdnoise), rtol=1e-4)
    assert ok, msg
    # Gaussian: B * S * 2^-24 * sum |x| per bin
    x = rc.cube(rng, B, S, N, "normal")
    snr, prof = refine_host(x, d, p, w, stdnoise, profiles=True)
    ref, mag = rc.numpy_profiles(x, d, p)
    assert np.all(np.abs(prof.astype(np.float64) - ref) <= B * S * 2.0 ** -24 * mag)
    ok, msg = snr_close(snr.reshape(-1, w.size), oracle.snr2(prof.reshape(-1, N), w, stdnoise), rtol=1e-4)
    assert ok, msg
    assert np.array_equal(refine_host(x, d, p, w, stdnoise), snr)       # without the profile output


@pytest.mark.parametrize("B,S,N,K,J", rc.OFFSET_SHAPES)
def test_host_snr_with_an_offset(B, S, N, K, J):
    """Profiles about 100 B S high: (h + b) * dmax - b * sum cancels most of
    two large terms, and the S/N is compared by the rounding of those terms
    (rc.snr1_bound), not by its own size.  The numpy restatement of refine_snr1
    gives the host's bits, and the host is within the bound of the expression
    in float64: the bound the device is held to (test_gpu_refine.py) is not
    too tight.  Largest |error| / bound of the host: 0.115 at (8, 8, 64), 0.081
    at (3, 2, 700)."""
    from riptide_amd.refine import refine_host
    g = rc.offset_job(B, S, N, K, J)
    assert list(g[3]) == [1, N // 3, N - 1] and g[4] == 1.7
    snr, prof = refine_host(*g, profiles=True)
    assert abs(float(prof.mean()) / (rc.OFFSET * B * S) - 1) < 0.01
    f32, f64, bound = rc.snr1_bound(prof, g[3], g[4])
    snr = snr.reshape(f32.shape)
    assert np.array_equal(snr.view(np.uint32), f32.view(np.uint32))
    ratio = np.abs(snr.astype(np.float64) - f64) / bound
    print(f"host S/N with an offset {(B, S, N)}: largest |error| / bound {ratio.max():.3f}, "
          f"largest |S/N| {np.abs(f64).max():.3f}, largest bound {bound.max():.3e}")
    assert (ratio <= 1.0).all(), ratio.max()


def test_workspace_bytes_of_a_batch():
    """rt_refine_workspace_bytes (host only): the descriptor table rounded up
    to 256 bytes, then y [K, S, N] floats per candidate; the planner's errors."""
    import ctypes
    from riptide_amd import _lib
    from riptide_amd.refine import pack_refine
    L = _lib.load()
    table = pack_refine(rc.batch_jobs())[3]
    shapes = rc.batch_shapes()
    assert table.size == rc.BATCH_SIZE == 40
    # the device's descriptor of a candidate (RefineCand, refine_host.hpp):
    # seven 64-bit offsets and twelve 32-bit fields
    entry = 7 * 8 + 12 * 4
    need = ctypes.c_size_t()
    _lib.check(L.rt_refine_workspace_bytes(_lib.ptr(table), table.size, ctypes.byref(need)))
    assert need.value == -(-table.size * entry // 256) * 256 + 4 * sum(K * S * N for _, S, N, K, _ in shapes)
    one = table[:1].copy()
    _lib.check(L.rt_refine_workspace_bytes(_lib.ptr(one), 1, ctypes.byref(need)))
    assert need.value == 256 + 4 * shapes[0][3] * shapes[0][1] * shapes[0][2]
    _lib.check(L.rt_refine_workspace_bytes(None, 0, ctypes.byref(need)))
    assert need.value == 0
    for field, bad, text in (("bins", 1, "bins must be in"), ("bins", 1025, "bins must be in"),
                             ("bands", 0, "must be >= 1"), ("subints", 0, "must be >= 1"), ("ndm", 0, "must be >= 1"),
                             ("nper", 0, "must be >= 1"), ("nw", 0, "no trial widths")):
        t = table.copy()
        t[field][17] = bad
        with pytest.raises(ValueError, match=text):
            _lib.check(L.rt_refine_workspace_bytes(_lib.ptr(t), t.size, ctypes.byref(need)))


def test_host_errors():
    from riptide_amd.refine import refine_host
    B, S, N = 2, 3, 5
    x = np.ones((B, S, N), dtype=np.float32)
    d, p = np.zeros((2, B), dtype=np.int32), np.zeros((2, S), dtype=np.int32)
    refine_host(x, d, p, [1, 4], 1.0)
    for tab, where, text in ((d, (1, 1), "DM shift outside"), (p, (1, 2), "period shift outside")):
        for bad in (N, -1):
            tab[where] = bad
            with pytest.raises(ValueError, match=text):
                refine_host(x, d, p, [1, 4], 1.0)
            tab[where] = 0
    for w in ([0, 1], [1, N]):
        with pytest.raises(ValueError, match="trial widths must be all > 0 and < columns"):
            refine_host(x, d, p, w, 1.0)
    for bad in (0.0, -2.0):
        with pytest.raises(ValueError, match="stdnoise must be > 0"):
            refine_host(x, d, p, [1, 4], bad)
    with pytest.raises(ValueError, match="no trial widths"):
        refine_host(x, d, p, [], 1.0)
    with pytest.raises(ValueError, match="dshift must be"):
        refine_host(x, d[:, :1], p, [1], 1.0)


@pytest.fixture(scope="module")
def recovery_tables():
    from riptide_amd.refine import refine_shifts
    periods, dms = rc.recovery_trials()
    pshift, dshift = refine_shifts(rc.R_PERIOD, rc.R_TOBS, rc.RN, rc.RS, rc.R_FREQS, rc.R_DM, periods, dms)
    return periods, dms, pshift, dshift


def test_recovery_host(recovery_tables):
    """The specification alone recovers (RK, RJ) on each of 20 seeds: what
    R_AMPLITUDE was chosen for."""
    from riptide_amd.refine import Refinement, refine_host
    periods, dms, pshift, dshift = recovery_tables
    assert not pshift[4].any() and not dshift[4].any() and pshift[rc.RJ].any() and dshift[rc.RK].any()
    for seed in range(20):
        x = rc.recovery_cube(seed, pshift, dshift)
        r = Refinement(periods, dms, rc.R_WIDTHS, refine_host(x, dshift, pshift, rc.R_WIDTHS, 8.0))
        assert r.best_index[:2] == (rc.RK, rc.RJ), (seed, r.best_index)
        assert r.best_snr > r.snr_map[4, 4]
        assert r.best_dm == dms[rc.RK] and r.best_period == periods[rc.RJ]


def test_refine_cube_host_defaults():
    from riptide_amd import Refinement, generate_width_trials, refine_cube
    from riptide_amd.refine import default_trials, refine_host, refine_shifts
    rng = np.random.RandomState(3)
    B, S, N = 4, 3, 32
    x = rng.normal(size=(B, S, N)).astype(np.float32)
    x[2] = 0.0                                               # a band with no unmasked channel
    f = np.array([1500.0, 1400.0, 1300.0, 1200.0])
    P, T = 0.25, 100.0
    r = refine_cube(x, f, P, T, 500.0, device=False)
    assert isinstance(r, Refinement)
    assert r.periods.shape == (33,) and r.dms.shape == (65,) and r.periods[16] == P and r.dms[32] == 500.0
    assert np.array_equal(r.widths, generate_width_trials(N))
    assert r.snr.shape == (65, 33, r.widths.size) and r.snr.dtype == np.float32
    assert np.array_equal(r.snr_map, r.snr.max(axis=2))
    pshift, dshift = refine_shifts(P, T, N, S, f, 500.0, r.periods, r.dms)
    # one bin per step: at the lowest band for DM, between the two ends of the span for period
    assert dshift[33, 3] == 1 and dshift[31, 3] == N - 1 and not dshift[32].any()
    assert list(pshift[19]) == [N - 1, 0, 1] and list(pshift[13]) == [1, 0, N - 1] and not pshift[16].any()
    snr, prof = refine_host(x, dshift, pshift, r.widths, np.sqrt(3.0), profiles=True)
    assert np.array_equal(snr, r.snr)                        # stdnoise = sqrt(live bands)
    k, j, w = np.unravel_index(np.argmax(snr), snr.shape)    # first maximum of the flat array
    assert (r.best_dm, r.best_period, r.best_width) == (r.dms[k], r.periods[j], r.widths[w])
    assert r.best_snr == snr[k, j, w] and r.best_index == (k, j, w)
    assert r.profile.dtype == np.float32 and np.array_equal(r.profile, prof[k, j])
    # DM trials below zero are dropped
    pd, dd = default_trials(P, T, N, f, 500.0)
    step = dd[1] - dd[0]
    low = refine_cube(x, f, P, T, 2.5 * step, device=False)
    assert low.dms.size == 32 + 3 and low.dms.min() >= 0 and np.isclose(low.dms[2], 2.5 * step)
    # a 2-D cube is one sub-integration; explicit trials, widths and stdnoise
    flat = refine_cube(x[:, 0], f, P, T, 500.0, periods=[P], dms=[499.0, 500.0], widths=[1, 2], stdnoise=2.0,
                       device=False)
    assert flat.snr.shape == (2, 1, 2)
    _, d2 = refine_shifts(P, T, N, 1, f, 500.0, [P], [499.0, 500.0])
    assert np.array_equal(flat.snr, refine_host(x[:, :1], d2, np.zeros((1, 1), np.int32), [1, 2], 2.0))
    # a tie goes to the lowest flat index
    tie = Refinement([1.0, 2.0], [3.0, 4.0], [1, 2], np.array([[[1, 5], [5, 2]], [[5, 5], [0, 0]]], np.float32))
    assert tie.best_index == (0, 0, 1) and (tie.best_dm, tie.best_period, tie.best_width) == (3.0, 1.0, 2)


def test_candidate_round_trip_with_refined():
    from riptide_amd import Candidate, Refinement
    sub = np.zeros((4, 16), dtype=np.float32)
    bands = np.zeros((3, 4, 16), dtype=np.float32)
    freqs = np.array([395.0, 385.0, 372.0])
    plain = Candidate({"snr": 9.0}, {"dm": 5.0}, "peaks", sub, subbands=bands, band_freqs=freqs)
    assert plain.refined is None and "refined" not in plain.to_dict()
    assert Candidate.from_dict(plain.to_dict()).refined is None
    r = Refinement([0.5], [5.0], [1], np.ones((1, 1, 1), np.float32))
    c = Candidate({"snr": 9.0}, {"dm": 5.0}, "peaks", sub, subbands=bands, band_freqs=freqs, refined=r)
    d = c.to_dict()
    assert set(d) == {"params", "tsmeta", "peaks", "subints", "subbands", "band_freqs", "refined"}
    back = Candidate.from_dict(d)
    assert back.refined is r and back.params == {"snr": 9.0}


def test_refine_candidates_host():
    """refine_candidates: tobs = m * period with m of rt_fold_shape for the
    tsmeta's length; candidates without sub-bands are left alone."""
    from riptide_amd import Candidate, refine_candidates, refine_cube
    from riptide_amd.refine import candidate_tobs
    rng = np.random.RandomState(8)
    bands = rng.normal(size=(3, 4, 16)).astype(np.float32)
    freqs = np.array([395.0, 385.0, 372.0])
    meta = {"dm": 5.0, "tsamp": 1e-3, "tobs": 8.192}
    params = {"snr": 9.0, "period": 0.5, "dm": 5.0}
    a = Candidate(dict(params), meta, "peaks", bands.sum(axis=0), subbands=bands, band_freqs=freqs)
    b = Candidate(dict(params), meta, "peaks", bands.sum(axis=0))
    assert candidate_tobs(a) == 16 * 0.5 and candidate_tobs(a, nsamp=6000) == 12 * 0.5
    out = refine_candidates([a, b], device=False)
    assert out[0] is a and b.refined is None and a.params == params
    ref = refine_cube(bands, freqs, 0.5, 8.0, 5.0, device=False)
    assert np.array_equal(a.refined.snr, ref.snr) and np.array_equal(a.refined.dms, ref.dms)
    assert np.array_equal(a.refined.profile, ref.profile)


def test_asan_refine_check():
    """`make asan` builds build/asan/refine_check (g++, AddressSanitizer +
    UBSan, no HIP): rt_refine_shifts and rt_refine_host on exact-size heap
    arrays at the shapes above, and every error return."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "refine_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("refine_check OK")
