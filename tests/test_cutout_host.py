"""Pulse cutouts on the host: the specification rt_pulse_cutouts_host against a
plain numpy restatement (bit for bit, the order of the float additions
included), the geometry of cutout_jobs, the chunk planner of
build_pulse_candidates, and the argument refusals.  No device."""
import os
import subprocess

import numpy as np
import pytest

from cutout_common import (FLOAT_KINDS, KINDS, case_samples, edge_jobs, make_jobs, numpy_cutouts, replaced,
                           zero_dm_mean)
from dedisp_common import assert_same_bits

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NSAMP, NCHANS, R, MAXD = 700, 24, 3, 60


def _table(seed):
    # some entries below 0 and some above max_delay: clamped as they are read
    return np.random.RandomState(seed).randint(-8, MAXD + 9, size=(R, NCHANS)).astype(np.int32)


def _block_mask(seed, nsamp, nchans, t_origin, block_len=37):
    from riptide_amd.rfi import BlockMask
    rng = np.random.RandomState(seed)
    nblk = -(-(t_origin + nsamp) // block_len)
    return BlockMask(rng.rand(nblk, nchans) < 0.2, block_len, rng.randint(0, 4, size=nchans).astype(np.float64))


@pytest.mark.parametrize("variant", ["plain", "mask", "zero_dm", "block_mask", "all"])
@pytest.mark.parametrize("kind", KINDS)
def test_host_equals_numpy(kind, variant):
    from riptide_amd import pulse_candidates as pc
    zero_dm = variant in ("zero_dm", "all")
    data, vals, nbits = case_samples(3, NSAMP, NCHANS, kind, exact_floats=zero_dm)
    delays = _table(4)
    jobs = edge_jobs(NSAMP, NCHANS, R)
    mask = (np.arange(NCHANS) % 5 == 1) if variant in ("mask", "all") else None
    bm, t_origin = None, 0
    if variant in ("block_mask", "all"):
        t_origin = 1234
        bm = _block_mask(5, NSAMP, NCHANS, t_origin)
        vals = replaced(vals, bm, t_origin, bm.typed_fill(vals.dtype, nbits))
    mean = zero_dm_mean(vals, mask) if zero_dm else None
    ref = numpy_cutouts(vals, jobs, delays, MAXD, kind in FLOAT_KINDS, mask, mean)
    got = pc.pulse_cutouts_host(data, jobs, delays, MAXD, mask=mask, zero_dm=zero_dm, nbits=nbits, block_mask=bm,
                                t_origin=t_origin)
    assert_same_bits(got, ref, f"{kind} {variant}")
    # the windows outside the block, the empty band
    for i in (3, 4, 6):
        o = int(jobs["out_off"][i])
        assert not got[o:o + int(jobs["nbins"][i])].any()
    assert got.any()


def test_host_fully_masked_band_and_out_argument():
    from riptide_amd import pulse_candidates as pc
    data, vals, _ = case_samples(1, 300, 8, "uint8")
    delays = np.zeros((1, 8), dtype=np.int32)
    jobs = make_jobs([(0, 2, 16, 0, 2, 5), (0, 2, 16, 0, 0, 8)])
    mask = np.zeros(8, dtype=bool)
    mask[2:5] = True
    out = np.full(40, 7.0, dtype=np.float32)
    got = pc.pulse_cutouts_host(data, jobs, delays, 0, mask=mask, out=out)
    assert got is out and not out[:16].any() and np.all(out[32:] == 7.0)
    keep = vals[:32].astype(np.int64).reshape(16, 2, 8).sum(axis=1)[:, ~mask].sum(axis=1)
    assert np.array_equal(out[16:32], keep.astype(np.float32))


def test_cutout_jobs_geometry():
    from riptide_amd import pulse_candidates as pc
    from riptide_amd.dedispersion import KDM, band_edges, dispersion_delays
    from riptide_amd.single_pulse import SinglePulse
    freqs = 1500.0 - 300.0 / 64 * np.arange(64)
    tsamp = 64e-6
    pulses = [SinglePulse(1.0, 5000, 60.0, 3, 9, 12.0, 5, 55.0, 65.0),
              SinglePulse(2.0, 9000, 2.0, 0, 1, 9.0, 2, 0.0, 4.0)]
    plan = pc.cutout_jobs(pulses, freqs, tsamp, nbins=128, nbands=16, ndm=33)
    assert plan.jobs.dtype == pc.CUTOUT_JOB_DTYPE and plan.jobs.shape == (2 * (16 + 33),)
    jobs = plan.jobs.reshape(2, 49)
    # centring: f = max(1, width // 2), the pulse's sample in bin nbins // 2
    assert list(plan.factors) == [4, 1] and list(plan.starts) == [5000 - 256, 9000 - 64]
    for p in range(2):
        assert np.all(jobs[p]["factor"] == plan.factors[p]) and np.all(jobs[p]["start"] == plan.starts[p])
        assert (pulses[p].sample - plan.starts[p]) // plan.factors[p] == 64
        assert np.all(jobs[p]["nbins"] == 128)
        # the frequency-time rows: band_edges at the pulse's own delay row
        assert np.array_equal(np.stack([jobs[p]["band_lo"][:16], jobs[p]["band_hi"][:16]], axis=1),
                              band_edges(64, 16))
        assert np.all(jobs[p]["delay_row"][:16] == p * 34)
        # the DM-time rows: the whole band, one delay row per DM of the grid
        assert np.all(jobs[p]["band_lo"][16:] == 0) and np.all(jobs[p]["band_hi"][16:] == 64)
        assert np.array_equal(jobs[p]["delay_row"][16:], p * 34 + 1 + np.arange(33))
    assert np.array_equal(np.sort(plan.jobs["out_off"]), np.arange(98) * 128)
    # the default span: the DM offset whose sweep across the band is half the window
    sweep = KDM * (freqs.min() ** -2 - freqs.max() ** -2)
    span0 = (128 * 4 / 2) * tsamp / sweep
    assert np.allclose(plan.dms[0], np.linspace(60.0 - span0, 60.0 + span0, 33), rtol=0, atol=1e-12)
    assert plan.dms[0][16] == pytest.approx(60.0)
    d_edge = dispersion_delays(freqs, [span0], tsamp)[0][0]
    assert abs(int(d_edge.max()) - 128 * 4 // 2) <= 1
    # clipped at DM 0: evenly spaced from 0 to dm + span
    span1 = (128 * 1 / 2) * tsamp / sweep
    assert span1 > 2.0
    assert np.allclose(plan.dms[1], np.linspace(0.0, 2.0 + span1, 33), rtol=0, atol=1e-12) and plan.dms[1][0] == 0.0
    # the delay table: dispersion_delays of [dm, grid] per pulse
    want, md = dispersion_delays(freqs, np.concatenate([[60.0], plan.dms[0], [2.0], plan.dms[1]]), tsamp)
    assert np.array_equal(plan.delays, want) and plan.delays.dtype == np.int32 and plan.max_delay == md
    # explicit span and factor; one DM; no pulses
    plan = pc.cutout_jobs(pulses[:1], freqs, tsamp, nbins=10, nbands=1, ndm=5, dm_span=100.0, factor=3)
    assert np.allclose(plan.dms[0], np.linspace(0.0, 160.0, 5)) and plan.starts[0] == 5000 - 15
    assert pc.cutout_jobs(pulses[:1], freqs, tsamp, ndm=1).dms[0, 0] == 60.0
    assert pc.cutout_jobs([], freqs, tsamp).jobs.size == 0
    with pytest.raises(ValueError, match="nsub must be in"):
        pc.cutout_jobs(pulses, freqs, tsamp, nbands=65)
    with pytest.raises(ValueError, match="nbins and ndm"):
        pc.cutout_jobs(pulses, freqs, tsamp, ndm=0)
    assert "not tuned" in pc.cutout_jobs.__doc__


def test_chunk_planner():
    from riptide_amd import pulse_candidates as pc
    rng = np.random.RandomState(9)
    lo = rng.randint(0, 100000, size=60)
    spans = np.stack([lo, lo + rng.randint(1, 3000, size=60)], axis=1)
    spans[7] = (500, 500)      # reads nothing: in no chunk
    row_bytes = 64
    for cap_rows in (3000, 5000, 20000, 200000):
        chunks = pc.plan_chunks(spans, row_bytes, cap_rows * row_bytes + 13)
        seen = []
        for a, b, idx in chunks:
            assert (b - a) * row_bytes <= cap_rows * row_bytes + 13      # the byte cap
            for i in idx:
                assert a <= spans[i, 0] and spans[i, 1] <= b             # covers every pulse it holds
            assert a == min(spans[i, 0] for i in idx) and b == max(spans[i, 1] for i in idx)
            seen += idx
        assert sorted(seen) == [i for i in range(60) if i != 7]          # every pulse exactly once
        firsts = [spans[i, 0] for i in seen]
        assert firsts == sorted(firsts)                                  # by first row read
    assert len(pc.plan_chunks(spans, row_bytes, 200000 * row_bytes)) == 1
    assert len(pc.plan_chunks(spans, row_bytes, 3000 * row_bytes)) >= 4
    with pytest.raises(ValueError, match="pulse 3 reads 2999 rows"):
        big = spans.copy()
        big[3] = (10, 3009)
        pc.plan_chunks(big, row_bytes, 2998 * row_bytes)
    with pytest.raises(ValueError, match="SinglePulse\\(time"):
        from riptide_amd.single_pulse import SinglePulse
        p = SinglePulse(1.0, 5000, 60.0, 3, 9, 12.0, 5, 55.0, 65.0)
        pc.plan_chunks([[0, 100]], 64, 6399, names=[repr(p)])


def test_refusals():
    from riptide_amd import pulse_candidates as pc
    data = np.ones((64, 8), dtype=np.uint8)
    delays = np.zeros((2, 8), dtype=np.int32)

    def call(row, md=10, zero_dm=False, d=delays, x=data):
        return pc.pulse_cutouts_host(x, make_jobs([row]), d, md, zero_dm=zero_dm)

    assert call((0, 2, 32, 1, 0, 8)).shape == (32,)
    for row, text in [((0, 0, 32, 1, 0, 8), "factor and nbins must be at least 1"),
                      ((0, 2, 0, 1, 0, 8), "factor and nbins must be at least 1"),
                      ((0, 2, 32, 2, 0, 8), "delay_row 2 is not below the 2 rows"),
                      ((0, 2, 32, 1, 5, 4), r"band \[5, 4\) is not a channel range"),
                      ((0, 2, 32, 1, 0, 9), r"band \[0, 9\) is not a channel range lo <= hi <= 8"),
                      ((0, 1 << 21, 1, 1, 0, 8), r"\(band_hi - band_lo\) \* factor \* 255 must be below 2\^31"),
                      ((0, 1 << 30, 2, 1, 0, 0), r"nbins \* factor samples must be below 2\^31"),
                      ((1 << 41, 1, 1, 1, 0, 8), "start is outside")]:
        with pytest.raises(ValueError, match=text):
            call(row)
    assert call((0, 1 << 20, 1, 1, 0, 8))[0] == 64 * 8      # 8 * 2^20 * 255 < 2^31
    assert call((0, 1 << 21, 1, 1, 0, 8), zero_dm=True)[0] == 0.0   # a float sum has no such limit
    with pytest.raises(ValueError, match="max_delay is outside"):
        call((0, 2, 32, 1, 0, 8), md=-1)
    with pytest.raises(ValueError, match=r"delays must be \[R, nchans\]"):
        call((0, 2, 32, 1, 0, 8), d=np.zeros((2, 7), dtype=np.int32))
    with pytest.raises(ValueError, match="at least 1"):
        call((0, 2, 32, 0, 0, 8), d=np.zeros((0, 8), dtype=np.int32))
    with pytest.raises(ValueError, match="block is empty"):
        call((0, 2, 32, 1, 0, 8), x=np.ones((0, 8), dtype=np.uint8))
    with pytest.raises(ValueError, match="CUTOUT_JOB_DTYPE"):
        pc.pulse_cutouts_host(data, np.zeros(3), delays, 10)
    jobs = make_jobs([(0, 2, 32, 1, 0, 8)])
    with pytest.raises(ValueError, match="out must be a contiguous float32 array of at least 32"):
        pc.pulse_cutouts_host(data, jobs, delays, 10, out=np.zeros(31, dtype=np.float32))
    jobs["out_off"] = 1
    with pytest.raises(ValueError, match="at least 33"):
        pc.pulse_cutouts_host(data, jobs, delays, 10, out=np.zeros(32, dtype=np.float32))
    # the entry point's own check of a job's bins against out
    from riptide_amd import _lib
    rc = _lib.load().rt_pulse_cutouts_host(_lib.ptr(data), 0, 64, 8, _lib.ptr(delays), 2, 10, None, _lib.ptr(jobs), 1,
                                           _lib.ptr(np.zeros(32, dtype=np.float32)), 32, 0, None)
    assert rc == _lib.RT_EINVAL
    with pytest.raises(ValueError, match="job 0: its bins reach past the 32 floats of out"):
        _lib.check(rc)
    assert pc.pulse_cutouts_host(data, make_jobs([]), delays, 10).shape == (0,)


def test_plan_rule():
    from riptide_amd import engine
    assert engine.pulse_cutouts_plan(1, 0, 4096) == (256, 1024, True)
    assert engine.pulse_cutouts_plan(1, 1, 4097) == (256, 1025, False)
    assert engine.pulse_cutouts_plan(1, 3, 4096) == (256, 1024, True)
    assert engine.pulse_cutouts_plan(4, 7, 1031) == (256, 1024, True)
    assert engine.pulse_cutouts_plan(4, 7, 1032) == (256, 1025, False)
    with pytest.raises(ValueError, match="esize must be 1"):
        engine.pulse_cutouts_plan(2, 0, 4)


def test_candidate_record():
    import riptide_amd
    from riptide_amd.single_pulse import SinglePulse
    assert riptide_amd.PulseCandidate is riptide_amd.pulse_candidates.PulseCandidate
    assert callable(riptide_amd.build_pulse_candidates)
    p = SinglePulse(1.25, 1250, 20.0, 2, 9, 13.5, 4, 10.0, 30.0)
    ft = np.arange(12, dtype=np.float32).reshape(3, 4)
    ft[1] = 5.0
    dt = np.array([[0, 0, 10, 0, 1, -1, 0, 2]], dtype=np.float32)
    c = riptide_amd.PulseCandidate(p, ft, dt, [20.0], [1400.0, 1300.0, 1200.0], 4, -0.5, 1e-3)
    d = c.to_dict()
    assert set(d) == {"pulse", "freq_time", "dm_time", "dms", "band_freqs", "factor", "t0", "tbin"}
    q = riptide_amd.PulseCandidate.from_dict(d)
    assert q.pulse == p and np.array_equal(q.freq_time, ft) and q.factor == 4 and q.t0 == -0.5
    n = c.normalised()
    assert np.array_equal(c.freq_time, ft)                       # a copy
    row = ft[0].astype(np.float64)
    mad = np.median(np.abs(row - np.median(row)))
    assert np.allclose(n.freq_time[0], (row - np.median(row)) / (1.4826 * mad))
    assert not n.freq_time[1].any()                              # a constant row: centred only
    assert n.dm_time[0, 2] == pytest.approx((10 - 0.0) / (1.4826 * 0.5))


def test_asan_cutout_check():
    """`make asan` builds build/asan/cutout_check (g++, AddressSanitizer +
    UBSan, no HIP): rt_pulse_cutouts_host on exact-size heap arrays (windows
    before, across and behind the block, every sample type, an empty band, a
    bin longer than the block, the zero-DM filter with a block mask) and every
    error return."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "cutout_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("cutout_check OK")
