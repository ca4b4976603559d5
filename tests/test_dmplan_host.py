"""CPU-only tests of the DM plan: the planner (rt_dm_plan) against its own
formulas restated in numpy, grouping and sharding, every refusal of the
planner and of the step table, the decimated specification
(rt_dedisperse_ds_host) against the numpy restatement at every sample type,
the dispatcher on two fake ranks, and the sanitizer build of the checker."""
import os
import socket
import subprocess

import numpy as np
import pytest

import dedisp_common as dc
import dmplan_common as dp
from conftest import REPO

BANDS = {
    "lband": (1600.0 - 0.390625 * np.arange(1024), 64e-6, 1000.0),
    "uhf": (300.0 + (100.0 / 4096) * np.arange(4096), 256e-6, 300.0),     # ascending
    "two": (np.array([400.0, 380.0]), 1e-3, 2000.0),
}


@pytest.fixture(scope="module")
def dd():
    from riptide_amd import dedispersion
    return dedispersion


@pytest.fixture(scope="module")
def engine():
    from riptide_amd import engine
    return engine


# ---------------------------------------------------------------- the planner

@pytest.mark.parametrize("name", sorted(BANDS))
@pytest.mark.parametrize("dm_min", [0.0, 12.5])
def test_touching_radii(dd, name, dm_min):
    freqs, tsamp, dm_max = BANDS[name]
    wmin = 1e-3
    plan = dd.dm_plan(freqs, tsamp, dm_max, dm_min=dm_min, wmin=wmin)
    dms = plan.dms
    kdisp, ksmear = dp.plan_quantities(freqs)
    r = dp.smear(dms, ksmear, wmin) / kdisp
    assert len(plan) == dms.size >= 2 and dms[0] == dm_min
    assert np.all(np.diff(dms) > 0)
    gap = np.abs((dms[1:] - r[1:]) - (dms[:-1] + r[:-1]))
    assert np.all(gap <= 1e-9 * np.maximum(1.0, dms[1:])), float(gap.max())
    assert dms[-1] + r[-1] >= dm_max > dms[-2] + r[-2]


@pytest.mark.parametrize("name", sorted(BANDS))
@pytest.mark.parametrize("oversample,max_downsamp", [(2.0, 64), (1.0, 8), (3.5, 256)])
def test_decimation_rule(dd, name, oversample, max_downsamp):
    freqs, tsamp, dm_max = BANDS[name]
    wmin = 1e-3
    plan = dd.dm_plan(freqs, tsamp, dm_max, wmin=wmin, oversample=oversample, max_downsamp=max_downsamp)
    _, ksmear = dp.plan_quantities(freqs)
    s = dp.smear(plan.dms, ksmear, wmin)
    f = plan.downsamp
    assert f.shape == plan.dms.shape
    assert np.all(f >= 1) and np.all(f <= max_downsamp) and np.all(f & (f - 1) == 0)
    assert np.all(np.diff(f) >= 0)
    fits = f * (tsamp * oversample) <= s
    assert np.all(fits | (f == 1))
    assert np.all((f == max_downsamp) | ~((2 * f) * (tsamp * oversample) <= s))
    if name == "lband" and max_downsamp == 64:
        # 1 ms over 2 x 64 us: 4 at DM 0; the 1.2 ms smearing of DM 1000 allows 8
        assert f[0] == 4 and f[-1] == 8


def test_grouping_and_sharding(dd):
    freqs, tsamp, dm_max = BANDS["lband"]
    plan = dd.dm_plan(freqs, tsamp, dm_max, wmin=1e-4)
    f = plan.downsamp
    # steps are the maximal runs of equal f
    runs = np.split(np.arange(f.size), np.flatnonzero(np.diff(f)) + 1)
    assert [s.dms.size for s in plan.steps] == [r.size for r in runs] and len(runs) >= 3
    assert [s.downsamp for s in plan.steps] == [int(f[r[0]]) for r in runs]
    assert all(s.tsamp == s.downsamp * tsamp for s in plan.steps)
    assert np.array_equal(np.concatenate([s.dms for s in plan.steps]), plan.dms)
    for n in (1, 2, 3, 7):
        seen = []
        for r in range(n):
            part = plan.shard(r, n)
            assert part.dm_cover == plan.dm_cover == plan.dms.max()
            assert all(s.dms.size for s in part.steps)
            by_f = {s.downsamp: s.dms for s in part.steps}
            for s in plan.steps:
                assert np.array_equal(by_f.get(s.downsamp, np.empty(0)), s.dms[r::n])
            idx = plan.shard_indices(r, n)
            assert np.array_equal(plan.dms[idx], part.dms)
            seen += idx
        assert sorted(seen) == list(range(len(plan)))
    tiny = dd.DMPlan.from_steps([([1.0], 1), ([2.0, 3.0], 5)])
    assert [s.dms.size for s in tiny.shard(1, 2).steps] == [1] and len(tiny.shard(1, 2)) == 1


def test_from_steps_takes_any_factor_in_range(dd):
    plan = dd.DMPlan.from_steps([([0.0, 1.0], 1), ([5.0], 37), ([], 4), ([9.0], 256)], tsamp=1e-3)
    assert [s.downsamp for s in plan.steps] == [1, 37, 256] and len(plan) == 4
    assert plan.steps[1].tsamp == 37e-3 and list(plan.downsamp) == [1, 1, 37, 256]
    for bad in (0, 257, 2.5):
        with pytest.raises(ValueError, match=r"must be an integer in \[1, 256\]"):
            dd.DMPlan.from_steps([([1.0], bad)])


PLANNER_REFUSALS = [
    (dict(freqs=[400.0]), "dm_plan: at least 2 channels are needed"),
    (dict(freqs=[400.0, -1.0]), "dm_plan: channel frequencies must be positive and finite"),
    (dict(freqs=[400.0, np.inf]), "dm_plan: channel frequencies must be positive and finite"),
    (dict(freqs=[400.0, 400.0]), "dm_plan: the channels must span a band above 0 MHz"),
    (dict(tsamp=0.0), "dm_plan: tsamp must be positive and finite"),
    (dict(tsamp=np.nan), "dm_plan: tsamp must be positive and finite"),
    (dict(wmin=-1e-3), "dm_plan: wmin must be positive and finite"),
    (dict(oversample=0.0), "dm_plan: oversample must be positive and finite"),
    (dict(kdm=np.inf), "dm_plan: kdm must be positive and finite"),
    (dict(dm_min=-1.0), "dm_plan: dm_min must be non-negative and finite"),
    (dict(dm_min=20.0, dm_max=10.0), "dm_plan: dm_max must be finite and at least dm_min"),
    (dict(dm_max=np.inf), "dm_plan: dm_max must be finite and at least dm_min"),
    (dict(max_downsamp=0), r"max_downsamp must be an integer in \[1, 256\]"),
    (dict(max_downsamp=512), r"max_downsamp must be an integer in \[1, 256\]"),
    (dict(freqs=np.linspace(400.0, 368.0, 1 << 20), wmin=1e-6, dm_max=1000.0), "dm_plan: more than 2\\^20 trials"),
]


@pytest.mark.parametrize("change,message", PLANNER_REFUSALS)
def test_planner_refusals(dd, change, message):
    kw = dict(freqs=dc.band(16), tsamp=1e-3, dm_max=100.0)
    kw.update(change)
    with pytest.raises(ValueError, match=message):
        dd.dm_plan(**kw)


def _step(engine, **kw):
    base = dict(delays_off=0, out_off=0, out_stride=240, out_offset=0, ndm=3, max_delay=10, downsamp=4, reserved=0)
    base.update(kw)
    return np.array([tuple(base[n] for n in engine.DEDISP_STEP_DTYPE.names)], dtype=engine.DEDISP_STEP_DTYPE)


STEP_REFUSALS = [
    (dict(downsamp=0), {}, r"dedisperse: downsamp 0 is outside \[1, 256\]"),
    (dict(downsamp=257), {}, r"dedisperse: downsamp 257 is outside \[1, 256\]"),
    (dict(max_delay=250), {}, "step 0: max_delay 250 is not below the 250 decimated samples of the block"),
    (dict(reserved=1), {}, "step 0: reserved must be 0"),
    (dict(ndm=0), {}, "step 0: ndm must be at least 1"),
    (dict(delays_off=1), {}, "step 0: its delay table leaves the delay array"),
    (dict(out_stride=239), {}, "step 0: out_stride is shorter than out_offset plus the step's outputs"),
    (dict(out_offset=1, out_stride=240), {}, "step 0: out_stride is shorter than out_offset plus the step's outputs"),
    (dict(out_off=1, out_stride=240), {}, "step 0: its output rows leave the output array"),
    (dict(), dict(t_origin=6), "block_mask: t_origin 6 is not a multiple of downsamp 4"),
    (dict(), dict(dtype="float64"), "the sample type must be"),
    (dict(), dict(nsamp_blk=1 << 31), "dedisperse: a block must be below 2\\^31 samples"),
]


@pytest.mark.parametrize("change,call,message", STEP_REFUSALS)
def test_step_table_refusals(engine, change, call, message):
    """nsamp_blk 1000 at downsamp 4: 250 decimated samples, 240 outputs at max_delay 10."""
    kw = dict(dtype="uint8", nsamp_blk=1000, nchans=16, delays_len=48, out_floats=3 * 240)
    engine.dedisperse_steps_check(steps=_step(engine), **kw)
    engine.dedisperse_steps_check(steps=_step(engine), t_origin=8, **kw)
    with pytest.raises(ValueError, match="a step table needs at least one step"):
        engine.dedisperse_steps_check(steps=np.empty(0, dtype=engine.DEDISP_STEP_DTYPE), **kw)
    kw.update(call)
    with pytest.raises(ValueError, match=message):
        engine.dedisperse_steps_check(steps=_step(engine, **change), **kw)


@pytest.mark.parametrize("kind,vmax", [("uint8", 255), ("int8", 255), ("u1", 1), ("u2", 3), ("u4", 15)])
def test_exactness_cap(dd, engine, kind, vmax):
    """Refused from the first channel count with vmax * f * nchans >= 2^24,
    accepted one below (whole bytes of packed rows; the 8-bit channel cap of
    the plain call still holds, which only f = 256 at 1 bit reaches first)."""
    f = 256
    per = 8 // int(kind[1:]) if kind.startswith("u") and kind != "uint8" else 1
    first = -(-(1 << 24) // (vmax * f))
    first = -(-first // per) * per
    ok = first - per
    assert vmax * f * ok < 1 << 24 <= vmax * f * first
    if kind == "uint8":
        assert ok == 257
    nbits = None if kind in ("uint8", "int8") else int(kind[1:])
    for nchans, refused in ((ok, False), (first, True)):
        st = _step(engine, downsamp=f, ndm=1, max_delay=0, out_stride=2)
        x = np.zeros((2 * f, nchans // per), dtype=np.int8 if kind == "int8" else np.uint8)
        delays = np.zeros((1, nchans), dtype=np.int64)
        if nchans > 65793:          # the plain call's cap comes first
            with pytest.raises(ValueError, match="too many channels for an exact 8-bit sum"):
                engine.dedisperse_steps_check(kind, 2 * f, nchans, st, nchans, 2)
            continue
        if refused:
            text = f"{nchans} channels at downsamp 256 are too many for an exact sum \\({vmax} \\* downsamp \\* nchans"
            with pytest.raises(ValueError, match=text):
                engine.dedisperse_steps_check(kind, 2 * f, nchans, st, nchans, 2)
            with pytest.raises(ValueError, match=text):
                dd.dedisperse_ds_host(x, delays, 0, f, nbits=nbits)
            # the zero-DM path sums in float32: no cap of its own
            engine.dedisperse_steps_check(kind, 2 * f, nchans, st, nchans, 2, zero_dm=True)
        else:
            engine.dedisperse_steps_check(kind, 2 * f, nchans, st, nchans, 2)
            assert dd.dedisperse_ds_host(x, delays, 0, f, nbits=nbits).shape == (1, 2)


# ---------------------------------------------------------------- the host specification

def _case(kind, nsamp, nchans, seed):
    rng = np.random.RandomState(seed)
    x, vals, nbits = dc.kind_samples(rng, nsamp, nchans, kind)
    mask = rng.rand(nchans) < 0.3
    mask[0] = False
    return x, vals, nbits, mask


@pytest.mark.parametrize("kind", dp.KINDS)
@pytest.mark.parametrize("nsamp", [97, 1000, 1003])
def test_host_equals_numpy_restatement(dd, kind, nsamp):
    for nchans in (2, 70):
        if kind.startswith("u") and kind != "uint8" and nchans * int(kind[1:]) % 8:
            nchans = 72 if nchans == 70 else 8          # whole bytes of packed rows
        x, vals, nbits, mask = _case(kind, nsamp, nchans, nsamp + nchans)
        for f in (1, 2, 3, 4, 5, 8):
            nz = nsamp // f
            delays = dp.delay_table(5, nchans, min(40, nz // 3), base=0)
            md = int(delays.max())
            nout = nz - md
            assert nout > 0
            for use_mask in (False, True):
                for zero_dm in (False, True):
                    m = mask if use_mask else None
                    got = dd.dedisperse_ds_host(x, delays, md, f, mask=m, zero_dm=zero_dm, nbits=nbits)
                    ref = dp.numpy_dedisperse_ds(vals, delays, f, nout, m, zero_dm)
                    dc.assert_same_bits(got, ref, f"{kind} nsamp {nsamp} nchans {nchans} f {f} mask {use_mask} "
                                                  f"zero_dm {zero_dm}")
                    if f == 1:
                        dc.assert_same_bits(got, dd.dedisperse_host(x, delays, md, mask=m, zero_dm=zero_dm,
                                                                    nbits=nbits), "f = 1 is dedisperse_host")
            # a shorter nout is the head of the full one
            short = dd.dedisperse_ds_host(x, delays, md, f, nout=nout // 2, nbits=nbits)
            dc.assert_same_bits(short, np.ascontiguousarray(dd.dedisperse_ds_host(x, delays, md, f,
                                                                                  nbits=nbits)[:, :nout // 2]))


@pytest.mark.parametrize("f", [2, 3, 4, 5, 8])
def test_decimated_sum_is_the_sum_of_native_outputs(dd, f):
    """uint8 data, native delays all multiples of f: out_f[d, u] is exactly
    the sum of the f native outputs it covers."""
    nsamp, nchans = 1003, 70
    x, _, _, mask = _case("uint8", nsamp, nchans, f)
    dec = dp.delay_table(4, nchans, 30, base=1)
    md = int(dec.max())
    nout = nsamp // f - md
    got = dd.dedisperse_ds_host(x, dec, md, f, mask=mask)
    native = dd.dedisperse_host(x, dec * f, md * f, mask=mask, nout=nout * f)
    assert np.array_equal(got, native.reshape(4, nout, f).sum(axis=2, dtype=np.float64).astype(np.float32))


def test_host_block_mask_is_a_replacement_in_front(dd):
    nsamp, nchans, f = 1000, 70, 4
    x, _, _, mask = _case("uint8", nsamp, nchans, 9)
    rng = np.random.RandomState(3)
    cells = (rng.rand(-(-(nsamp + 8) // 37), nchans) < 0.2).astype(np.uint8)
    fill = rng.randint(0, 256, nchans).astype(np.uint8)
    delays = dp.delay_table(3, nchans, 20)
    md = int(delays.max())
    got = dd.dedisperse_ds_host(x, delays, md, f, mask=mask, block_mask=(cells, fill, 37), t_origin=8)
    flag = np.repeat(cells, 37, axis=0)[8:8 + nsamp].astype(bool)
    ref = dd.dedisperse_ds_host(np.where(flag, fill[None, :], x).astype(np.uint8), delays, md, f, mask=mask)
    dc.assert_same_bits(got, ref)
    assert not np.array_equal(got, dd.dedisperse_ds_host(x, delays, md, f, mask=mask))
    with pytest.raises(ValueError, match="block_mask: t_origin 6 is not a multiple of downsamp 4"):
        dd.dedisperse_ds_host(x, delays, md, f, block_mask=(cells, fill, 37), t_origin=6)


def test_host_refusals(dd):
    x = np.zeros((100, 4), dtype=np.uint8)
    delays = np.zeros((1, 4), dtype=np.int64)
    with pytest.raises(ValueError, match=r"downsamp 0 is outside \[1, 256\]"):
        dd.dedisperse_ds_host(x, delays, 0, 0)
    with pytest.raises(ValueError, match="nout \\+ max_delay exceeds the 33 decimated samples of the input"):
        dd.dedisperse_ds_host(x, delays, 0, 3, nout=34)
    with pytest.raises(ValueError, match="a delay is outside \\[0, max_delay\\]"):
        dd.dedisperse_ds_host(x, delays + 2, 1, 3)


# ---------------------------------------------------------------- the dispatcher on two fake ranks

class _FakeSearcher:
    """EngineSearcher.search_filterbank_plan's contract without a GPU: per DM
    two peaks carrying the step's factor (width), the plan's dm_cover (ip,
    rounded) and the DM."""

    def search_filterbank_plan(self, fb, plan, mask=None, kdm=None, zero_dm=False, block_mask=None):
        from riptide_amd.peak_detection import Peak
        return [[Peak(0.5 + k, 1.0 / (0.5 + k), s.downsamp, 0.01, 1, int(round(plan.dm_cover)), 9.0, float(dm))
                 for k in range(2)] for s in plan.steps for dm in s.dms]


def _fake_fb(path):
    from riptide_amd.reading import Filterbank, write_sigproc
    x = np.random.RandomState(5).randint(0, 256, size=(3000, 8)).astype(np.uint8)
    header = {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": 1e-3, "nbits": 8,
              "fch1": 400.0, "foff": -4.0, "nchans": 8, "nifs": 1}
    write_sigproc(str(path), x, header)
    return Filterbank(str(path))


def _fake_plan():
    from riptide_amd.dedispersion import DMPlan
    return DMPlan.from_steps([([0.0, 2.0, 4.0], 1), ([10.0, 12.0, 14.0, 16.0, 18.0], 2), ([30.0], 8)], tsamp=1e-3)


def _plan_worker(rank, world, port, fname, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import riptide_amd
        peaks = riptide_amd.search_filterbank_plan(fname, _fake_plan(), _FakeSearcher())
        q.put((rank, [tuple(p) for p in peaks]))
    finally:
        dist.destroy_process_group()


def test_search_filterbank_plan_order_and_two_ranks(tmp_path):
    import torch.multiprocessing as mp
    import riptide_amd
    fb = _fake_fb(tmp_path / "fake.fil")
    plan = _fake_plan()
    single = riptide_amd.search_filterbank_plan(fb, plan, _FakeSearcher(), group=None)
    # plan order, then range order; every rank's shard keeps the plan's cover
    assert [(p.dm, p.period) for p in single] == [(dm, 0.5 + k) for dm in plan.dms for k in range(2)]
    assert [p.width for p in single[::2]] == list(plan.downsamp)
    assert {p.ip for p in single} == {30}
    assert riptide_amd.search_filterbank_plan(fb, riptide_amd.DMPlan.from_steps([]), _FakeSearcher()) == []
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_plan_worker, args=(r, 2, port, fb.fname, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert results[0] == results[1] == [tuple(p) for p in single]


def test_plan_layout_covers_one_stretch_whatever_the_shard(dd, tmp_path):
    fb = _fake_fb(tmp_path / "fake.fil")
    plan = _fake_plan()
    whole = dd.plan_layout(fb, plan)
    _, D = dd.dispersion_delays(fb.freqs, [30.0], fb.tsamp)
    for (delays, md, nout), s in zip(whole, plan.steps):
        assert nout == min((fb.nsamp - D) // s.downsamp, fb.nsamp // s.downsamp - md)
        assert np.array_equal(delays, dc.numpy_delays(fb.freqs, s.dms, fb.tsamp * s.downsamp))
    part = plan.shard(1, 2)
    by_f = {s.downsamp: nout for (_, _, nout), s in zip(whole, plan.steps)}
    assert [nout for _, _, nout in dd.plan_layout(fb, part)] == [by_f[s.downsamp] for s in part.steps]


def test_plan_slices_fit_the_budget_and_keep_the_cover(dd, tmp_path):
    fb = _fake_fb(tmp_path / "fake.fil")
    plan = _fake_plan()
    whole = dd.plan_device_bytes(fb, plan)
    assert whole > 0 and dd.plan_device_bytes(fb, dd.DMPlan.from_steps([])) == 0
    assert [len(p) for p in dd.plan_slices(fb, plan, whole, chunk=2)] == [len(plan)]
    budget = whole - 1          # the fixed part, the gulp buffers and the workspace, is most of this small file's
    parts = dd.plan_slices(fb, plan, budget, chunk=2)
    assert len(parts) > 1 and all(dd.plan_device_bytes(fb, p) <= budget for p in parts)
    assert np.array_equal(np.concatenate([p.dms for p in parts]), plan.dms)
    assert np.array_equal(np.concatenate([p.downsamp for p in parts]), plan.downsamp)
    assert all(p.dm_cover == plan.dm_cover and p.tsamp == plan.tsamp for p in parts)
    # a slice's rows are as long as the whole plan's
    by_f = {s.downsamp: nout for (_, _, nout), s in zip(dd.plan_layout(fb, plan), plan.steps)}
    for p in parts:
        assert [nout for _, _, nout in dd.plan_layout(fb, p)] == [by_f[s.downsamp] for s in p.steps]
    with pytest.raises(ValueError, match="dedispersing 2 DMs of the plan needs .* over the budget of 1000"):
        dd.plan_slices(fb, plan, 1000, chunk=2)


def test_a_plan_of_another_sampling_time_is_refused(dd, tmp_path):
    fb = _fake_fb(tmp_path / "fake.fil")
    other = dd.DMPlan.from_steps([([0.0, 2.0], 1), ([10.0], 2)], tsamp=2e-3)
    with pytest.raises(ValueError, match="the plan was made for a sampling time of 0.002 s, the file has 0.001 s"):
        dd.plan_layout(fb, other)
    assert len(dd.plan_layout(fb, dd.DMPlan.from_steps([([0.0, 2.0], 1), ([10.0], 2)]))) == 2      # no tsamp: no claim


def test_asan_dmplan_check():
    """`make asan` builds build/asan/dmplan_check (g++, AddressSanitizer +
    UBSan, no HIP): rt_dm_plan, rt_dedisperse_ds_host and the step table's
    checks on exact-size heap arrays at the edge shapes of these tests."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "dmplan_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("dmplan_check OK")


def test_injected_pulsar_clears_the_threshold_at_the_decimated_resolution(dd, oracle):
    """The fixture of the GPU end-to-end test, on the CPU: the host
    specification at the plan trial nearest the injected DM (f = 4) and the
    oracle periodogram find the 0.5 s train far above the search's S/N 7."""
    plan = dp.e2e_plan()
    k, dm_true = dp.e2e_true_dm(plan)
    f = int(plan.downsamp[k])
    assert f == 4 and abs(dm_true - 10.0) < 0.2
    x = dp.e2e_data(dm_true)
    tsamp = dp.E2E["tsamp"] * f
    delays, md = dd.dispersion_delays(dp.e2e_freqs(), [plan.dms[k]], tsamp)
    series = dd.dedisperse_ds_host(x, delays, md, f)[0]
    kw = dp.E2E_RANGES[0]["ffa_search"]
    widths = oracle.generate_width_trials(kw["bins_min"], 0.2)
    periods, _, snrs = oracle.periodogram(oracle.normalise(series), tsamp, widths, kw["period_min"],
                                          kw["period_max"], kw["bins_min"], kw["bins_max"])
    best = np.unravel_index(np.argmax(snrs), snrs.shape)
    print("best S/N", float(snrs[best]), "at period", float(periods[best[0]]))
    assert snrs[best] > 3 * 7.0
    assert abs(periods[best[0]] - dp.E2E["period"]) <= dp.e2e_period_step()
