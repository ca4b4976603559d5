"""GPU tests of the candidate refinement (refine_kernels.hip through rt_refine
and rt_refine_device): profiles bit for bit against the host specification at
every kernel path, batching, device tables that were never validated, recovery
of an off-centre trial, and a candidate refined straight from a file."""
import numpy as np
import pytest

import dedisp_common as dc
import refine_common as rc
from conftest import snr_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# (B, S, N, K, J): the smallest, odd sizes, around one wave and one block of
# bins, the widest profile, and the two sides of the 64 KiB LDS stage of stage
# B (S * N * 4 = 65536 and 67584); (32, 4, 255) and (5, 3, 257) take two bins
# per thread or an idle tail
SHAPES = [(1, 1, 2, 1, 1), (2, 1, 3, 3, 2), (7, 2, 63, 3, 3), (7, 2, 64, 3, 3), (7, 2, 65, 3, 3), (32, 4, 255, 2, 3),
          (5, 3, 257, 2, 2), (2, 2, 1024, 2, 2), (2, 32, 512, 3, 3), (2, 33, 512, 3, 3)]


def job(B, S, N, K, J, kind, seed=0):
    rng = np.random.RandomState(seed + B * 1000 + S * 10 + N)
    d, p = rc.tables(rng, B, S, N, K, J)
    return (rc.cube(rng, B, S, N, kind), d, p, rc.widths_for(N), 1.7)


@pytest.mark.parametrize("B,S,N,K,J", SHAPES)
def test_bit_identity(torch, B, S, N, K, J):
    from riptide_amd.refine import refine_host, refine_many
    g = job(B, S, N, K, J, "normal")
    if B > 1:
        assert g[1].max() == N - 1 and g[1].min() == 0       # 0 and N - 1 together
    if S > 1:
        assert g[2].max() == N - 1 and g[2].min() == 0
    assert g[3][0] == 1 and g[3][-1] == N - 1
    snr, prof = refine_many([g], profiles=True)[0]
    hsnr, hprof = refine_host(*g, profiles=True)
    assert prof.shape == (K, J, N) and np.array_equal(bits(prof), bits(hprof))
    ok, msg = snr_close(snr, hsnr, rtol=1e-4)
    assert ok, msg
    # small integers: exact against numpy
    g = job(B, S, N, K, J, "int")
    snr, prof = refine_many([g], profiles=True)[0]
    ref, _ = rc.numpy_profiles(g[0], g[1], g[2])
    assert np.array_equal(prof.astype(np.float64), ref)
    ok, msg = snr_close(snr, refine_host(*g), rtol=1e-4)
    assert ok, msg


def test_stage_a_global_path(torch):
    """A slice of stage A past the LDS stage (bands * bins * 4 > 64 KiB): the
    rows are read from global memory, the same bits."""
    from riptide_amd.refine import refine_host, refine_many
    g = job(33, 2, 512, 2, 2, "normal")
    snr, prof = refine_many([g], profiles=True)[0]
    hsnr, hprof = refine_host(*g, profiles=True)
    assert np.array_equal(bits(prof), bits(hprof))
    ok, msg = snr_close(snr, hsnr, rtol=1e-4)
    assert ok, msg


def test_batching(torch):
    """Five candidates of different shapes in one call equal each alone, bit
    for bit; without the profile output the S/N is unchanged."""
    from riptide_amd.refine import refine_many
    jobs = [job(*s, "normal", seed=7) for s in [(3, 2, 64, 2, 3), (1, 1, 2, 1, 1), (2, 33, 512, 2, 2), (7, 5, 257, 3, 1),
                                                (4, 4, 100, 1, 4)]]
    together = refine_many(jobs, profiles=True)
    for g, (snr, prof) in zip(jobs, together):
        s1, p1 = refine_many([g], profiles=True)[0]
        assert np.array_equal(bits(snr), bits(s1)) and np.array_equal(bits(prof), bits(p1))
    for (snr, _), alone in zip(together, refine_many(jobs)):
        assert np.array_equal(bits(snr), bits(alone))


def test_unvalidated_device_tables(torch):
    """engine.refine_device does not validate device tables: entries of N,
    2N + 1, -1 and INT32_MIN run, as (v mod 2^32) mod N.  No value is illegal:
    the kernel reduces each entry as it loads it."""
    from riptide_amd import engine
    from riptide_amd.refine import pack_refine, refine_host
    B, S, N, K, J = 5, 4, 100, 3, 3
    g = job(B, S, N, K, J, "normal", seed=3)
    d, p = g[1].copy(), g[2].copy()
    d[1, :4] = [N, 2 * N + 1, -1, -2 ** 31]
    p[2, :4] = [-2 ** 31, -1, 2 * N + 1, N]
    cubes, shifts, widths, table, _, nsnr, nprof = pack_refine([(g[0], d, p, g[3], g[4])])
    dev = "cuda"
    snr, prof = engine.refine_device(torch.from_numpy(cubes).to(dev), torch.from_numpy(shifts).to(dev),
                                     torch.from_numpy(widths.astype(np.int32)).to(dev), table, profiles=True)
    torch.cuda.synchronize()
    assert snr.numel() == nsnr and prof.numel() == nprof

    def reduced(t):
        return ((t.astype(np.int64) % 2 ** 32) % N).astype(np.int32)
    hsnr, hprof = refine_host(g[0], reduced(d), reduced(p), g[3], g[4], profiles=True)
    assert np.array_equal(bits(prof.cpu().numpy().reshape(K, J, N)), bits(hprof))
    ok, msg = snr_close(snr.cpu().numpy().reshape(hsnr.shape), hsnr, rtol=1e-4)
    assert ok, msg
    snr2, none = engine.refine_device(torch.from_numpy(cubes).to(dev), torch.from_numpy(shifts).to(dev),
                                      torch.from_numpy(widths.astype(np.int32)).to(dev), table)
    assert none is None and torch.equal(snr2, snr)
    with pytest.raises(ValueError, match="exceed the device tensors"):
        engine.refine_device(torch.from_numpy(cubes[:-1]).to(dev), torch.from_numpy(shifts).to(dev),
                             torch.from_numpy(widths.astype(np.int32)).to(dev), table)


def test_host_buffer_form_validates(torch):
    from riptide_amd.refine import refine_many
    g = job(2, 3, 5, 2, 2, "int")
    for k, bad, text in ((1, 5, "DM shift outside"), (2, -1, "period shift outside")):
        t = g[k].copy()
        t[1, 1] = bad
        with pytest.raises(ValueError, match=text):
            refine_many([g[:k] + (t,) + g[k + 1:]])
    with pytest.raises(ValueError, match="trial widths must be all > 0 and < columns"):
        refine_many([g[:3] + ([1, 5], 1.0)])
    with pytest.raises(ValueError, match="stdnoise must be > 0"):
        refine_many([g[:4] + (0.0,)])
    with pytest.raises(ValueError, match="bins must be in"):
        refine_many([(np.zeros((1, 1, 1025), np.float32), [[0]], [[0]], [1], 1.0)])


def test_recovery_device(torch):
    """The CPU recovery case (test_refine_host.py) through the kernels: the
    same argmax."""
    from riptide_amd.refine import Refinement, refine_host, refine_many, refine_shifts
    periods, dms = rc.recovery_trials()
    pshift, dshift = refine_shifts(rc.R_PERIOD, rc.R_TOBS, rc.RN, rc.RS, rc.R_FREQS, rc.R_DM, periods, dms)
    jobs = [(rc.recovery_cube(seed, pshift, dshift), dshift, pshift, rc.R_WIDTHS, 8.0) for seed in range(4)]
    for g, snr in zip(jobs, refine_many(jobs)):
        r = Refinement(periods, dms, rc.R_WIDTHS, snr)
        h = Refinement(periods, dms, rc.R_WIDTHS, refine_host(*g))
        assert r.best_index[:2] == (rc.RK, rc.RJ) and r.best_index == h.best_index
        assert r.best_snr > r.snr_map[4, 4]


# ------------------------------------------------------------- from a file
F_PERIOD, F_DM, F_NSUB, F_BINS = 0.5, 20.0, 8, 64
F_RANGES = [{"name": "short",
             "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
             "candidates": {"bins": F_BINS, "subints": 8}}]
F_DEREDDEN = {"rmed_width": 0.5, "rmed_minpts": 101}
# 8-sample pulses 6 units high over a channel noise of 10: folded over 65
# periods and a sub-band's 8 channels a bin of a sub-band holds the pulse at
# about 6 * 8 / 10 * sqrt(65 * 8 / 8) = 39 noise units, far above the trial to
# trial differences; the host specification is asserted on the same cube first
F_AMPLITUDE = 6.0
F_NOUT = 30000        # samples of every folded series: the largest delay here is a few hundred


def _pulse_filterbank(path):
    from test_gpu_dedisp import _write_filterbank
    nchans, nsamp = 64, 2 ** 15
    rng = np.random.RandomState(99)
    x = rng.normal(100.0, 10.0, size=(nsamp, nchans))
    sweep = dc.numpy_delays(dc.band(nchans), [F_DM], dc.TSAMP)[0]
    period = int(round(F_PERIOD / dc.TSAMP))
    for c in range(nchans):
        for t0 in range(100 + int(sweep[c]), nsamp - 8, period):
            x[t0:t0 + 8, c] += F_AMPLITUDE
    return _write_filterbank(path, np.clip(np.round(x), 0, 255).astype(np.uint8))


def test_refine_from_a_file(torch, tmp_path):
    import pandas  # noqa: F401  (Candidate.peaks is a DataFrame)
    from riptide_amd import Peak, PeakCluster, build_candidates_filterbank, refine_candidates
    from riptide_amd.dedispersion import band_edges
    from riptide_amd.reading import open_filterbank
    from riptide_amd.refine import default_trials
    fname = _pulse_filterbank(tmp_path / "r.fil")
    fb = open_filterbank(fname)
    band_freqs = np.array([fb.freqs[lo:hi].mean() for lo, hi in band_edges(fb.nchans, F_NSUB)])
    _, grid = default_trials(F_PERIOD, 30.0, F_BINS, band_freqs, F_DM)
    step = grid[1] - grid[0]
    dm0 = F_DM + 3.0 * step                  # the cluster: three default steps off the truth
    peak = Peak(period=F_PERIOD, freq=1.0 / F_PERIOD, width=3, ducy=3 / 64, iw=1, ip=0, snr=20.0, dm=dm0)
    plain = build_candidates_filterbank([PeakCluster([peak], rank=0)], fb, F_RANGES, F_DEREDDEN, nsub=F_NSUB,
                                        nout=F_NOUT)
    assert len(plain) == 1 and plain[0].refined is None            # the default is unchanged
    cands = build_candidates_filterbank([PeakCluster([peak], rank=0)], fb, F_RANGES, F_DEREDDEN, nsub=F_NSUB,
                                        nout=F_NOUT, refine=True)
    c = cands[0]
    assert c.subbands.shape == (F_NSUB, 8, F_BINS) and np.array_equal(c.subbands, plain[0].subbands)
    assert c.params["dm"] == dm0 and c.params["period"] == F_PERIOD

    def conditions(r):
        kc = int(np.argmin(np.abs(r.dms - dm0)))
        jc = int(np.argmin(np.abs(r.periods - F_PERIOD)))
        assert r.dms[kc] == dm0 and r.periods[jc] == F_PERIOD
        assert abs(r.best_dm - F_DM) < abs(dm0 - F_DM), (r.best_dm, dm0)
        assert abs(r.best_dm - F_DM) <= step * (1 + 1e-9), (r.best_dm, step)
        assert r.best_snr >= r.snr_map[kc, jc]

    # the host specification on the same cube meets the conditions ...
    host = refine_candidates([plain[0]], device=False, nsamp=F_NOUT)[0].refined
    conditions(host)
    # ... and so does the device
    dev = c.refined
    conditions(dev)
    assert np.array_equal(dev.dms, host.dms) and np.array_equal(dev.periods, host.periods)
    assert dev.snr.shape == (dev.dms.size, 33, dev.widths.size)
    ok, msg = snr_close(dev.snr, host.snr, rtol=1e-4)
    assert ok, msg
    assert dev.best_index == host.best_index and np.array_equal(bits(dev.profile), bits(host.profile))
