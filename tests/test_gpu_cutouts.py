"""GPU tests of the pulse cutouts: engine.pulse_cutouts_device against the host
specification (pulse_candidates.pulse_cutouts_host), bit for bit, at the
shapes where the kernel can go wrong -- channel counts around a step of 8
channels and a wave, bin counts around the tile of 256, factors up to a bin
longer than a tile, every sample type and option, every window edge, both
sides of the staged / direct boundary -- then build_pulse_candidates on a
synthetic file and `cutouts=` of search_filterbank_pulses."""
import numpy as np
import pytest

import dedisp_common as dc
from cutout_common import KINDS, case_samples, edge_jobs, make_jobs

pytestmark = pytest.mark.gpu

DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def device_block_mask(torch, bm, fill):
    from riptide_amd import engine
    if fill.dtype == np.uint16:
        fill = fill.view(np.int16)       # the same bits
    return engine.DeviceBlockMask(torch.from_numpy(bm.cells.astype(np.uint8)).cuda(), torch.from_numpy(fill).cuda(),
                                  bm.block_len)


def assert_device_is_host(torch, data, jobs, delays, max_delay, nbits=None, mask=None, zero_dm=False, bm=None,
                          t_origin=0, **kw):
    """One device call against the specification: the same bits.  Returns them."""
    from riptide_amd import engine, pulse_candidates as pc
    ref = pc.pulse_cutouts_host(data, jobs, delays, max_delay, mask=mask, zero_dm=zero_dm, nbits=nbits,
                                block_mask=bm, t_origin=t_origin)
    d_bm = None
    if bm is not None:
        d_bm = device_block_mask(torch, bm, np.ascontiguousarray(bm.typed_fill(np.asarray(data).dtype, nbits)))
    got = engine.pulse_cutouts_device(torch.from_numpy(np.ascontiguousarray(data)).cuda(), jobs,
                                      torch.from_numpy(np.ascontiguousarray(delays, dtype=np.int32)).cuda(),
                                      max_delay, mask=None if mask is None else torch.from_numpy(
                                          np.asarray(mask).astype(np.uint8)).cuda(),
                                      zero_dm=zero_dm, nbits=nbits, block_mask=d_bm, t_origin=t_origin, **kw)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    dc.assert_same_bits(got[:ref.size], ref)
    return got


def spread_table(rng, R, nchans, max_delay):
    """Delays spread over [0, max_delay], with a negative entry and one above
    max_delay in every row (both clamped as they are read)."""
    d = rng.randint(0, max_delay + 1, size=(R, nchans)).astype(np.int32)
    d[:, 0] = -5
    d[:, -1] = max_delay + 1000
    if nchans > 2:
        d[:, 1] = max_delay
    return d


@pytest.mark.parametrize("kind", ["uint8", "float32"])
@pytest.mark.parametrize("nchans", [1, 63, 65, 130])
def test_shapes(torch, nchans, kind):
    """Every T in {1, 63, 64, 65, 256, 257} with every f in {1, 2, 3, 7, 64,
    300} in one launch: bins below, at and above a wave and the tile, factors
    from one sample to a bin longer than a tile; channel counts of a single
    channel, one short of and one past a multiple of the 8-channel step and of
    a wave, and more than two waves."""
    nsamp = 3000
    data, _, nbits = case_samples(nchans, nsamp, nchans, kind)
    rng = np.random.RandomState(nchans)
    delays = spread_table(rng, 4, nchans, 700)
    rows = []
    for T in (1, 63, 64, 65, 256, 257):
        for f in (1, 2, 3, 7, 64, 300):
            rows.append((int(rng.randint(-200, 1500)), f, T, int(rng.randint(0, 4)), 0, nchans))
    got = assert_device_is_host(torch, data, make_jobs(rows), delays, 700, nbits=nbits)
    assert np.count_nonzero(got) > got.size // 2


@pytest.mark.parametrize("variant", ["plain", "mask", "zero_dm", "block_mask", "all"])
@pytest.mark.parametrize("kind", KINDS)
def test_types_options_and_window_edges(torch, kind, variant):
    """Every sample type with each of the channel mask, the zero-DM filter and
    a block mask (a block length that divides neither tile, a non-zero
    t_origin), on the jobs of cutout_common.edge_jobs: a window that starts
    before the block, ends past it, lies wholly outside it (zeros), crosses
    its end for the delayed channels only; an empty, a partial, an
    overlapping and the whole band."""
    from riptide_amd.rfi import BlockMask
    nsamp, nchans, R, max_delay = 2048, 65, 3, 60
    zero_dm = variant in ("zero_dm", "all")
    data, _, nbits = case_samples(11, nsamp, nchans if kind not in ("u1", "u2", "u4") else 72, kind,
                                  exact_floats=zero_dm)
    nchans = data.shape[1] * 8 // nbits if nbits else data.shape[1]
    delays = spread_table(np.random.RandomState(12), R, nchans, max_delay)
    jobs = edge_jobs(nsamp, nchans, R)
    mask = (np.arange(nchans) % 5 == 1) if variant in ("mask", "all") else None
    bm, t_origin = None, 0
    if variant in ("block_mask", "all"):
        rng = np.random.RandomState(13)
        t_origin, block_len = 1234, 37
        nblk = -(-(t_origin + nsamp) // block_len)
        bm = BlockMask(rng.rand(nblk, nchans) < 0.2, block_len, rng.randint(0, 4, size=nchans).astype(np.float64))
    got = assert_device_is_host(torch, data, jobs, delays, max_delay, nbits=nbits, mask=mask, zero_dm=zero_dm, bm=bm,
                                t_origin=t_origin)
    for i in (3, 4, 6):    # wholly outside the block, and the empty band
        o = int(jobs["out_off"][i])
        assert not got[o:o + int(jobs["nbins"][i])].any()


def test_fully_masked_band(torch):
    data, _, _ = case_samples(2, 2048, 65, "int8")
    delays = spread_table(np.random.RandomState(3), 2, 65, 100)
    mask = np.zeros(65, dtype=bool)
    mask[8:24] = True
    jobs = make_jobs([(50, 3, 300, 0, 8, 24), (50, 3, 300, 1, 0, 65), (50, 3, 300, 1, 7, 25)])
    got = assert_device_is_host(torch, data, jobs, delays, 100, mask=mask)
    assert not got[:300].any() and got[300:].any()


def paths(jobs, delays, max_delay, nsamp, nchans, esize):
    """The set of paths ('S' staged, 'D' direct) the channels of every (job,
    tile) take, named by engine.pulse_cutouts_plan from the clamped spans."""
    from riptide_amd import engine
    seen = set()
    d = np.clip(delays, 0, max_delay)
    for job in jobs:
        f, T = int(job["factor"]), int(job["nbins"])
        for t0 in range(0, T, 256):
            nb = min(256, T - t0)
            for c in range(int(job["band_lo"]), int(job["band_hi"])):
                a = int(job["start"]) + t0 * f + int(d[int(job["delay_row"]), c])
                lo, hi = max(a, 0), min(a + nb * f, nsamp)
                if lo < hi:
                    tile, ndw, staged = engine.pulse_cutouts_plan(esize, lo, hi)
                    assert tile == 256
                    seen.add(("S" if staged else "D", ndw))
    return seen


@pytest.mark.parametrize("kind", ["uint8", "int8", "float32"])
def test_staged_direct_boundary(torch, kind):
    """A channel's span of a tile is staged in LDS up to 1024 dwords.  8-bit
    rows: 256 bins of 16 samples are exactly 4096 bytes, staged where the
    channel's first sample is dword-aligned and direct where it is not, so a
    delay table whose entries take every residue mod 4, spread over hundreds
    of samples, puts neighbouring channels of one step on both paths with some
    exactly at the limit; f = 15 is staged and f = 17 direct for every
    channel.  Float rows: 256 bins of 4 samples are exactly 1024 dwords, f = 5
    is direct, and a direct window that the block's end cuts short is staged
    again.  A negative entry and one above max_delay are clamped."""
    esize = 4 if kind == "float32" else 1
    nsamp, nchans, max_delay = 4096 + 900, 21, 600
    data, _, _ = case_samples(5, nsamp, nchans, kind)
    rng = np.random.RandomState(6)
    delays = spread_table(rng, 2, nchans, max_delay)
    delays[0, 2:10] = [0, 1, 2, 3, 597, 598, 599, 600]      # every residue, at both ends of the spread
    fs = (15, 16, 17) if esize == 1 else (3, 4, 5)
    rows = [(40, f, 256, 0, 0, nchans) for f in fs]
    rows += [(41, fs[1], 256, 1, 0, nchans), (nsamp - 300 - 600, fs[2], 256, 0, 0, nchans),
             (-17, fs[1], 300, 1, 3, nchans)]
    jobs = make_jobs(rows)
    seen = paths(jobs, delays, max_delay, nsamp, nchans, esize)
    assert ("S", 1024) in seen and {p for p, _ in seen} == {"S", "D"}, seen
    if esize == 1:
        assert ("D", 1025) in seen
        one = paths(jobs[1:2], delays, max_delay, nsamp, nchans, esize)
        assert {p for p, _ in one} == {"S", "D"}      # both paths inside one job's steps
    assert {p for p, _ in paths(jobs[0:1], delays, max_delay, nsamp, nchans, esize)} == {"S"}
    assert {p for p, _ in paths(jobs[2:3], delays, max_delay, nsamp, nchans, esize)} == {"D"}
    assert_device_is_host(torch, data, jobs, delays, max_delay)
    assert_device_is_host(torch, data, jobs, delays, max_delay, zero_dm=(kind != "float32"))


@pytest.mark.parametrize("kind,zero_dm", [("uint8", False), ("int8", False), ("float32", False), ("uint8", True),
                                          ("u2", False), ("u16", False)])
def test_whole_band_equals_dedisperse(torch, kind, zero_dm):
    """The whole-band row at f = 1 is the matching slice of
    engine.dedisperse_device, bit for bit."""
    from riptide_amd import engine
    from riptide_amd.dedispersion import dispersion_delays
    nchans, nsamp = 64, 2500
    delays, max_delay = dispersion_delays(dc.band(nchans), [0.0, 20.0, 50.0], dc.TSAMP)
    data, _, nbits = case_samples(8, nsamp, nchans, kind)
    nout = nsamp - max_delay
    jobs = make_jobs([(0, 1, nout, 2, 0, nchans), (700, 1, 300, 1, 0, nchans), (5, 1, 257, 0, 0, nchans)])
    got = assert_device_is_host(torch, data, jobs, delays, max_delay, nbits=nbits, zero_dm=zero_dm)
    series = engine.dedisperse_device(torch.from_numpy(data).cuda(), torch.from_numpy(delays.astype(np.int32)).cuda(),
                                      max_delay, zero_dm=zero_dm, nbits=nbits).cpu().numpy()
    dc.assert_same_bits(got[:nout], series[2])
    dc.assert_same_bits(got[nout:nout + 300], series[1, 700:1000])
    dc.assert_same_bits(got[nout + 300:], series[0, 5:262])


def test_job_lists(torch):
    """About 50 jobs of mixed f, T and bands in one launch; no jobs; out
    supplied (longer than needed: the rest untouched) and allocated; a side
    stream; a workspace of the caller."""
    from riptide_amd import engine
    nsamp, nchans = 4096, 130
    data, _, _ = case_samples(21, nsamp, nchans, "uint8")
    rng = np.random.RandomState(22)
    delays = spread_table(rng, 7, nchans, 500)
    rows = []
    for _ in range(50):
        lo = int(rng.randint(0, nchans))
        rows.append((int(rng.randint(-300, nsamp)), int(rng.choice([1, 2, 3, 5, 8, 21, 64, 130])),
                     int(rng.choice([1, 17, 64, 200, 256, 300, 513])), int(rng.randint(0, 7)), lo,
                     int(rng.randint(lo, nchans + 1))))
    jobs = make_jobs(rows)
    got = assert_device_is_host(torch, data, jobs, delays, 500)
    need = got.size
    out = torch.full((need + 9,), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(engine.dedisperse_workspace_bytes("uint8", nsamp, nchans) + 64, dtype=torch.uint8, device="cuda")
    again = assert_device_is_host(torch, data, jobs, delays, 500, out=out, workspace=ws)
    assert np.array_equal(again[:need], got) and np.all(again[need:] == 7.0)
    side = torch.cuda.Stream()
    streamed = assert_device_is_host(torch, data, jobs, delays, 500, stream=side)
    assert np.array_equal(streamed, got)
    # jobs in another order write the same floats
    perm = rng.permutation(jobs.size)
    assert np.array_equal(assert_device_is_host(torch, data, jobs[perm], delays, 500), got)
    block, d = torch.from_numpy(data).cuda(), torch.from_numpy(delays).cuda()
    none = engine.pulse_cutouts_device(block, make_jobs([]), d, 500)
    assert tuple(none.shape) == (0,) and none.dtype == torch.float32
    assert engine.pulse_cutouts_device(block, make_jobs([]), d, 500, out=out) is out


def test_device_refusals(torch):
    from riptide_amd import engine
    block = torch.zeros((64, 8), dtype=torch.uint8, device="cuda")
    d = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    ok = make_jobs([(0, 2, 32, 1, 0, 8)])
    assert engine.pulse_cutouts_device(block, ok, d, 10).shape == (32,)
    for row, text in [((0, 0, 32, 1, 0, 8), "factor and nbins"), ((0, 2, 32, 2, 0, 8), "delay_row 2"),
                      ((0, 2, 32, 1, 0, 9), "not a channel range"),
                      ((0, 1 << 21, 1, 1, 0, 8), r"factor \* 255 must be below 2\^31")]:
        with pytest.raises(ValueError, match=text):
            engine.pulse_cutouts_device(block, make_jobs([row]), d, 10)
    with pytest.raises(ValueError, match="delays must be a contiguous int32"):
        engine.pulse_cutouts_device(block, ok, d.long(), 10)
    with pytest.raises(ValueError, match="out must be a contiguous float32"):
        engine.pulse_cutouts_device(block, ok, d, 10, out=torch.zeros(31, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="workspace must be"):
        engine.pulse_cutouts_device(block, ok, d, 10, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="mask must be"):
        engine.pulse_cutouts_device(block, ok, d, 10, mask=torch.zeros(7, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="CUTOUT_JOB_DTYPE"):
        engine.pulse_cutouts_device(block, np.zeros(2), d, 10)


# ---- the filterbank front end

NCHANS, NSAMP = 64, 16384
TRUE_DM, T0, WIDTH = 30.0, 8000, 8        # a dispersed pulse: its sample at the top of the band, its width
SPIKE = 3000                              # an undispersed spike of two samples


def header(nbits):
    return {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": dc.TSAMP,
            "nbits": nbits, "fch1": 400.0, "foff": -32.0 / NCHANS, "nchans": NCHANS, "nifs": 1}


@pytest.fixture(scope="module")
def two_bit_values():
    """Values 0 .. 3 (so that a 2-bit file holds them too): noise of sigma 0.8
    per channel, a dispersed pulse of one count at DM 30 and a spike of two
    counts at DM 0."""
    rng = np.random.RandomState(97)
    x = rng.normal(1.2, 0.8, size=(NSAMP, NCHANS))
    sweep = dc.numpy_delays(dc.band(NCHANS), [TRUE_DM], dc.TSAMP)[0]
    for c in range(NCHANS):
        x[T0 + int(sweep[c]):T0 + int(sweep[c]) + WIDTH, c] += 1.0
    x[SPIKE:SPIKE + 2] += 2.0
    return np.clip(np.round(x), 0, 3).astype(np.uint8)


def candidate_pulses():
    from riptide_amd.single_pulse import SinglePulse
    return [SinglePulse((T0 + WIDTH // 2) * dc.TSAMP, T0 + WIDTH // 2, TRUE_DM, 3, WIDTH, 20.0, 5, 20.0, 40.0),
            SinglePulse(SPIKE * dc.TSAMP, SPIKE, 10.0, 1, 2, 15.0, 3, 0.0, 20.0),
            SinglePulse(0.02, 20, 40.0, 4, 6, 9.0, 1, 40.0, 40.0),                 # its window starts before the file
            SinglePulse((NSAMP - 30) * dc.TSAMP, NSAMP - 30, 25.0, 2, 12, 9.0, 1, 25.0, 25.0),   # and ends past it
            SinglePulse(12.0, 12000, 5.0, 0, 1, 8.5, 1, 5.0, 5.0)]


def test_build_pulse_candidates(torch, tmp_path, two_bit_values):
    """On a 16384 x 64 file of 8-bit samples: the candidates are the
    specification's on the whole file in memory; one chunk, five chunks and
    the 2-bit file of the same values give identical arrays; a pulse that
    does not fit chunk_bytes is refused by name; and the cutouts show what
    was injected."""
    import riptide_amd
    from riptide_amd import pulse_candidates as pc
    from riptide_amd.reading import PackedFilterbank, pack_samples, write_sigproc
    x = two_bit_values
    path8, path2 = str(tmp_path / "eight.fil"), str(tmp_path / "two.fil")
    write_sigproc(path8, x, header(8))
    write_sigproc(path2, pack_samples(x, 2).ravel(), header(2))
    fb = riptide_amd.open_filterbank(path8)
    pulses = candidate_pulses()
    kw = dict(nbins=128, nbands=16, ndm=32)
    cands = riptide_amd.build_pulse_candidates(fb, pulses, **kw)
    assert [c.pulse for c in cands] == pulses
    plan = pc.cutout_jobs(pulses, fb.freqs, fb.tsamp, **kw)
    ref = pc.pulse_cutouts_host(x, plan.jobs, plan.delays, plan.max_delay).reshape(len(pulses), 48, 128)
    for i, c in enumerate(cands):
        assert c.freq_time.shape == (16, 128) and c.dm_time.shape == (32, 128)
        dc.assert_same_bits(c.freq_time, ref[i, :16])
        dc.assert_same_bits(c.dm_time, ref[i, 16:])
        assert np.array_equal(c.dms, plan.dms[i]) and c.factor == plan.factors[i]
        assert c.tbin == c.factor * fb.tsamp and c.t0 == plan.starts[i] * fb.tsamp
    # nothing in front of the file: the first bins of the top band, whose delays are a few samples
    assert cands[2].t0 < 0 and not cands[2].freq_time[0, :8].any() and cands[2].freq_time[0, 64:].all()
    # chunk_bytes: everything in one chunk, and every pulse in a chunk of its own
    spans = plan.spans(fb.nsamp)
    assert len(pc.plan_chunks(spans, NCHANS, 1 << 30)) == 1
    small = int((spans[:, 1] - spans[:, 0]).max()) * NCHANS
    assert len(pc.plan_chunks(spans, NCHANS, small)) >= 4
    fb2 = riptide_amd.open_filterbank(path2)
    assert isinstance(fb2, PackedFilterbank)
    for other in (riptide_amd.build_pulse_candidates(path8, pulses, chunk_bytes=small, **kw),
                  riptide_amd.build_pulse_candidates(fb2, pulses, **kw),
                  riptide_amd.build_pulse_candidates(fb2, pulses, chunk_bytes=small // 4, **kw)):
        for a, b in zip(cands, other):
            dc.assert_same_bits(a.freq_time, b.freq_time)
            dc.assert_same_bits(a.dm_time, b.dm_time)
    with pytest.raises(ValueError, match=r"SinglePulse\(time=.* reads \d+ rows of 64 bytes, more than chunk_bytes"):
        riptide_amd.build_pulse_candidates(fb, pulses, chunk_bytes=small - NCHANS, **kw)
    assert riptide_amd.build_pulse_candidates(fb, []) == []
    # options reach the kernel: the zero-DM filter and a channel mask, still the specification's bits
    mask = np.arange(NCHANS) % 7 == 0
    opt = riptide_amd.build_pulse_candidates(fb, pulses[:2], mask=mask, zero_dm=True, chunk_bytes=small, **kw)
    plan2 = pc.cutout_jobs(pulses[:2], fb.freqs, fb.tsamp, **kw)
    ref2 = pc.pulse_cutouts_host(x, plan2.jobs, plan2.delays, plan2.max_delay, mask=mask, zero_dm=True)
    dc.assert_same_bits(np.concatenate([np.concatenate([c.freq_time, c.dm_time]).ravel() for c in opt]), ref2)
    # what was injected: the dispersed pulse is straight at its DM and in the middle bin ...
    n = cands[0].normalised()
    assert abs(int(np.argmax(n.freq_time.sum(axis=0))) - 64) <= 1
    assert int(np.argmax(n.dm_time.max(axis=1))) == int(np.argmin(np.abs(cands[0].dms - TRUE_DM)))
    assert cands[0].dms[0] == 0.0 or cands[0].dms[0] < TRUE_DM < cands[0].dms[-1]
    # ... and the undispersed spike peaks in the DM 0 row of a pulse claimed at DM 10
    s = cands[1].normalised()
    assert cands[1].dms[0] == 0.0 and int(np.argmax(s.dm_time.max(axis=1))) == 0
    assert abs(int(np.argmax(s.dm_time[0])) - 64) <= 1


def test_search_filterbank_pulses_cutouts(torch, tmp_path):
    """cutouts={} returns one candidate per pulse, in pulse order, each the
    build_pulse_candidates of that pulse; without cutouts the call returns
    what it did."""
    import riptide_amd
    from riptide_amd.reading import write_sigproc
    rng = np.random.RandomState(2468)
    x = rng.normal(100.0, 10.0, size=(NSAMP, NCHANS))
    sweep = dc.numpy_delays(dc.band(NCHANS), [TRUE_DM], dc.TSAMP)[0]
    for t0, w, a in ((3000, 1, 30.0), (8000, 8, 12.0), (12000, 40, 5.0)):
        for c in range(NCHANS):
            x[t0 + int(sweep[c]):t0 + int(sweep[c]) + w, c] += a
    path = str(tmp_path / "pulses.fil")
    write_sigproc(path, np.clip(np.round(x), 0, 255).astype(np.uint8), header(8))
    dms = [0.0, 10.0, 20.0, 30.0, 40.0, 50.0]
    plain = riptide_amd.search_filterbank_pulses(path, dms, DEREDDEN, batch=3)
    assert isinstance(plain, tuple) and len(plain) == 2
    pulses, events, cands = riptide_amd.search_filterbank_pulses(path, dms, DEREDDEN, batch=3, cutouts={})
    assert pulses == plain[0] and np.array_equal(events, plain[1]) and len(pulses) >= 3
    assert len(cands) == len(pulses) and all(c.pulse == p for c, p in zip(cands, pulses))
    assert all(c.freq_time.shape == (64, 256) and c.dm_time.shape == (64, 256) for c in cands)
    direct = riptide_amd.build_pulse_candidates(path, pulses)
    for a, b in zip(cands, direct):
        dc.assert_same_bits(a.freq_time, b.freq_time)
        dc.assert_same_bits(a.dm_time, b.dm_time)
    top = cands[0].normalised()
    assert abs(int(np.argmax(top.freq_time.sum(axis=0))) - 128) <= 1
    few = riptide_amd.search_filterbank_pulses(path, dms, DEREDDEN, batch=3, cutouts={"nbins": 32, "ndm": 8})[2]
    assert all(c.dm_time.shape == (8, 32) for c in few)
    assert riptide_amd.search_filterbank_pulses(path, [], DEREDDEN, cutouts={})[2] == []
