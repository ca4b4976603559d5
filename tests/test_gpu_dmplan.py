"""GPU tests of the DM plan's dedispersion: dedisp_decimate_kernel and the
float32 sum over its rows against the host specification
(rt_dedisperse_ds_host) bit for bit, the step table in one call, the block
mask, gulp independence of dedisperse_filterbank_plan, a side stream, the
refusals, and the search of a decimated trial end to end."""
import numpy as np
import pytest

import dedisp_common as dc
import dmplan_common as dp

pytestmark = pytest.mark.gpu

FACTORS = (2, 3, 4, 8, 16, 37, 256)
NDM = 19          # one full DM tile and a ragged one


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _whole_bytes(nchans, kind):
    per = 8 // int(kind[1:]) if kind in ("u1", "u2", "u4") else 1
    return -(-nchans // per) * per


def _samples(seed, nsamp, nchans, kind, zero_dm):
    """Real floats for float32 data; under the zero-DM filter quarter
    integers, whose float64 channel sums are exact in any order, so the
    device's mean series is the host's."""
    rng = np.random.RandomState(seed)
    if kind == "float32" and zero_dm:
        x = (rng.randint(-40, 41, size=(nsamp, nchans)) * 0.25).astype(np.float32)
        return x, x, None
    return dc.kind_samples(rng, nsamp, nchans, kind)


def run_steps(torch, x, nbits, specs, mask=None, margin=0, gap=0, canary=None, stream=None, **kw):
    """engine.dedisperse_steps_device on steps [(delays int64, max_delay, f)]:
    (list of numpy [ndm, nout], the whole flat output as numpy, the table).
    Rows are gap floats apart beyond nout, with margin floats around every
    step's rows; canary pre-fills the output."""
    from riptide_amd import engine
    nsamp_blk = x.shape[0]
    table = np.zeros(len(specs), dtype=engine.DEDISP_STEP_DTYPE)
    row0, off = 0, margin
    for k, (delays, md, f) in enumerate(specs):
        nout = nsamp_blk // f - md
        table[k] = (row0 * delays.shape[1], off, nout + gap, 0, delays.shape[0], md, f, 0)
        row0 += delays.shape[0]
        off += delays.shape[0] * (nout + gap) + margin
    out = torch.full((off,), np.nan if canary is None else canary, dtype=torch.float32, device="cuda")
    d = _dev(torch, np.concatenate([s[0] for s in specs]).astype(np.int32))
    m = None if mask is None else _dev(torch, np.asarray(mask, dtype=np.uint8))
    views = engine.dedisperse_steps_device(_dev(torch, x), d, table, out, mask=m, nbits=nbits, stream=stream, **kw)
    if stream is not None:
        stream.synchronize()
    return [v.cpu().numpy() for v in views], out.cpu().numpy(), table


def _cases():
    """A few dozen of the product: every kind, factor, flag, channel count,
    block length and sum path at least once."""
    cases = []
    for i in range(28):
        kind = dp.KINDS[i % 7]
        f = FACTORS[(3 * i + i // 7) % 7]
        zero_dm, masked = bool(i % 2), bool((i // 2) % 2)
        nchans = _whole_bytes((70, 130)[(i // 3) % 2], kind)
        nsamp_blk = (4099, 16384 + 5)[(i // 2 + i // 7) % 2]
        if f == 256:
            nsamp_blk = 256 * 41 + 5
        nz = nsamp_blk // f
        wide = nz >= 700 and (i // 4) % 2 == 0   # a spread over 264 decimated samples needs the room
        cases.append((kind, f, zero_dm, masked, nchans, nsamp_blk, wide))
    # the staged 8-bit path with the bias of int8 rows, and in more than one piece (f = 100: 1600 dwords a wave)
    cases.append(("int8", 3, False, True, 70, 4099, False))
    cases.append(("int8", 37, False, False, 70, 16389, False))
    cases.append(("uint8", 100, False, False, 130, 16389, False))
    cases.append(("int8", 100, False, True, 70, 16389, False))
    return cases


CASES = _cases()


def test_cases_cover_every_axis():
    from riptide_amd import engine
    assert {c[0] for c in CASES} == set(dp.KINDS) and {c[1] for c in CASES} >= set(FACTORS)
    for axis in (2, 3, 6):
        assert {c[axis] for c in CASES} == {False, True}
    assert {c[4] for c in CASES} >= {70, 130, 72, 136} and all(c[4] % 64 for c in CASES)
    assert {c[5] for c in CASES} >= {4099, 16389}
    # the tail of the block is dropped, and some decimated lengths are no multiple of 4: the pitch padding is live
    assert all(c[5] % c[1] for c in CASES if c[1] in (2, 4, 8, 16, 256))
    assert sum(1 for c in CASES if (c[5] // c[1]) % 4) >= 8
    assert all(c[5] // c[1] >= 40 for c in CASES)
    # the two tables take the two paths of the float32 sum in the first DM tile's last channel
    for wide, staged in ((False, True), (True, False)):
        t = dp.delay_table(NDM, 70, 600 if wide else 40)[:16, -1]
        assert engine.dedisperse_span_plan(4, int(t.min()), int(t.max()))[1] is staged


@pytest.mark.parametrize("kind,f,zero_dm,masked,nchans,nsamp_blk,wide", CASES)
def test_device_equals_host_specification(torch, kind, f, zero_dm, masked, nchans, nsamp_blk, wide):
    from riptide_amd import dedispersion as dd
    x, vals, nbits = _samples(nsamp_blk + f, nsamp_blk, nchans, kind, zero_dm)
    nz = nsamp_blk // f
    delays = dp.delay_table(NDM, nchans, 600 if wide else min(40, nz // 3))
    md = int(delays.max())
    assert nz - md >= 1
    mask = None
    if masked:
        mask = np.random.RandomState(f).rand(nchans) < 0.3
        mask[-1] = False
    (got,), flat, _ = run_steps(torch, x, nbits, [(delays, md, f)], mask=mask, zero_dm=zero_dm, margin=64, gap=3)
    ref = dd.dedisperse_ds_host(x, delays, md, f, mask=mask, zero_dm=zero_dm, nbits=nbits)
    dc.assert_same_bits(got, ref, f"{kind} f {f}")
    # nothing but the outputs is written: the margins and the gap between rows keep their NaN
    assert int(np.isnan(flat).sum()) == flat.size - ref.size
    if kind not in ("float32", "u16") and not zero_dm:
        assert np.array_equal(got, np.rint(got))          # exact integers


def test_step_table_in_one_call(torch):
    from riptide_amd import engine
    nsamp_blk, nchans = 4099, 70
    for kind, zero_dm in (("uint8", False), ("int8", True), ("float32", False)):
        x, _, nbits = _samples(3, nsamp_blk, nchans, kind, zero_dm)
        specs = []
        for f in (1, 2, 8):
            d = dp.delay_table(NDM if f == 2 else 5, nchans, 40, base=f)
            specs.append((d, int(d.max()), f))
        mask = np.arange(nchans) % 7 == 3
        got, flat, table = run_steps(torch, x, nbits, specs, mask=mask, zero_dm=zero_dm, margin=32, gap=5, canary=-7.0)
        for k, spec in enumerate(specs):
            (alone,), _, _ = run_steps(torch, x, nbits, [spec], mask=mask, zero_dm=zero_dm)
            dc.assert_same_bits(got[k], alone, f"{kind} step {k}")
        d1, md1, _ = specs[0]
        plain = engine.dedisperse_device(_dev(torch, x), _dev(torch, d1.astype(np.int32)), md1,
                                         mask=_dev(torch, mask.astype(np.uint8)), zero_dm=zero_dm).cpu().numpy()
        dc.assert_same_bits(got[0], plain, "the f = 1 step is dedisperse_device")
        # the canaries: everything outside the steps' [ndm, nout] outputs is untouched
        written = np.zeros(flat.size, dtype=bool)
        for t, g in zip(table, got):
            for r in range(int(t["ndm"])):
                start = int(t["out_off"]) + r * int(t["out_stride"])
                written[start:start + g.shape[1]] = True
        assert np.all(flat[~written] == -7.0) and written.sum() == sum(g.size for g in got)


def test_host_buffer_form(torch):
    """rt_dedisperse_steps (dedispersion.dedisperse_steps): host arrays in, the
    three steps of one table out, the bits of the host specification; floats
    no step writes come back as they were; a delay above its step's max_delay
    is refused."""
    from riptide_amd import dedispersion as dd, engine
    nsamp, nchans = 4099, 70
    for kind, zero_dm in (("uint8", False), ("int8", True), ("float32", False), ("u2", False)):
        nch = _whole_bytes(nchans, kind)
        x, _, nbits = _samples(4, nsamp, nch, kind, zero_dm)
        specs = []
        for f in (1, 2, 8):
            d = dp.delay_table(NDM if f == 2 else 5, nch, 40, base=f)
            specs.append((d, int(d.max()), f))
        mask = np.arange(nch) % 7 == 3
        table = np.zeros(3, dtype=engine.DEDISP_STEP_DTYPE)
        row0, off, margin, gap = 0, 32, 32, 5
        for k, (d, md, f) in enumerate(specs):
            nout = nsamp // f - md
            table[k] = (row0 * nch, off, nout + gap, 0, d.shape[0], md, f, 0)
            row0 += d.shape[0]
            off += d.shape[0] * (nout + gap) + margin
        delays = np.concatenate([s[0] for s in specs])
        out = np.full(off, -7.0, dtype=np.float32)
        views = dd.dedisperse_steps(x, delays, table, out, mask=mask, zero_dm=zero_dm, nbits=nbits)
        written = np.zeros(out.size, dtype=bool)
        for v, t, (d, md, f) in zip(views, table, specs):
            ref = dd.dedisperse_ds_host(x, d, md, f, mask=mask, zero_dm=zero_dm, nbits=nbits)
            dc.assert_same_bits(np.ascontiguousarray(v), ref, f"{kind} f {f}")
            for r in range(d.shape[0]):
                start = int(t["out_off"]) + r * int(t["out_stride"])
                written[start:start + ref.shape[1]] = True
        assert np.all(out[~written] == -7.0) and int((~written).sum()) == 4 * margin + gap * (5 + NDM + 5)
        bad = delays.copy()
        bad[5 + NDM - 1, 3] = specs[1][1] + 1           # the second step's table, one past its max_delay
        before = out.copy()
        with pytest.raises(ValueError, match=r"a delay is outside \[0, max_delay\]"):
            dd.dedisperse_steps(x, bad, table, out, mask=mask, zero_dm=zero_dm, nbits=nbits)
        assert np.array_equal(out, before)
    with pytest.raises(ValueError, match="out must be a contiguous one-dimensional float32 array"):
        dd.dedisperse_steps(x, delays, table, out.astype(np.float64), nbits=nbits)


@pytest.mark.parametrize("kind", ["uint8", "u2", "float32"])
def test_block_mask_is_a_replacement_in_front(torch, kind):
    from riptide_amd import engine, rfi
    nsamp_blk, nchans, f, block_len, t_origin = 4099, 72, 4, 37, 8
    x, vals, nbits = _samples(11, nsamp_blk, nchans, kind, False)
    rng = np.random.RandomState(5)
    cells = rng.rand(-(-(t_origin + nsamp_blk) // block_len), nchans) < 0.2
    fill = (rng.randint(0, 4, nchans).astype(np.uint8) if kind != "float32"
            else rng.normal(size=nchans).astype(np.float32))
    specs = [(dp.delay_table(5, nchans, 30), None, 1), (dp.delay_table(NDM, nchans, 30), None, f)]
    specs = [(d, int(d.max()), ff) for d, _, ff in specs]
    bm = engine.DeviceBlockMask(_dev(torch, cells.astype(np.uint8)), _dev(torch, fill), block_len)
    xp = rfi.apply_block_mask_host(x, cells, block_len, fill, t_origin=t_origin, nbits=nbits)
    for zero_dm in (False, True):
        got, _, _ = run_steps(torch, x, nbits, specs, zero_dm=zero_dm, block_mask=bm, t_origin=t_origin)
        ref, _, _ = run_steps(torch, xp, nbits, specs, zero_dm=zero_dm)
        plain, _, _ = run_steps(torch, x, nbits, specs, zero_dm=zero_dm)
        for g, r, p in zip(got, ref, plain):
            dc.assert_same_bits(g, r, f"{kind} zero_dm {zero_dm}")
            assert not np.array_equal(g, p)


def _write(path, x, nbits=None):
    from riptide_amd.reading import pack_samples, write_sigproc
    nchans = x.shape[1]
    header = {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": dc.TSAMP,
              "nbits": 8 if nbits is None else nbits, "fch1": 400.0, "foff": -32.0 / nchans, "nchans": nchans,
              "nifs": 1}
    write_sigproc(str(path), x if nbits is None else pack_samples(x, nbits).ravel(), header)
    return str(path)


@pytest.mark.parametrize("nbits", [None, 2])
def test_filterbank_plan_does_not_depend_on_gulp(torch, tmp_path, nbits):
    from riptide_amd import dedispersion as dd
    from riptide_amd.reading import open_filterbank, pack_samples
    nsamp, nchans = 20000, 64
    rng = np.random.RandomState(8)
    x = rng.randint(0, 256 if nbits is None else 4, size=(nsamp, nchans)).astype(np.uint8)
    fb = open_filterbank(_write(tmp_path / "x.fil", x, nbits))
    plan = dd.DMPlan.from_steps([([0.0, 5.0, 10.0], 1), ([20.0, 30.0], 4), ([50.0, 60.0], 16)], tsamp=fb.tsamp)
    layout = dd.plan_layout(fb, plan)
    overlap = -(-max(md * s.downsamp for (_, md, _), s in zip(layout, plan.steps)) // 16) * 16
    assert overlap > 200
    mask = np.arange(nchans) % 9 == 4
    raw = x if nbits is None else pack_samples(x, nbits)
    for zero_dm in (False, True):
        one = [t.cpu().numpy() for t in dd.dedisperse_filterbank_plan(fb, plan, mask=mask, zero_dm=zero_dm)]
        small = [t.cpu().numpy() for t in dd.dedisperse_filterbank_plan(fb, plan, mask=mask, zero_dm=zero_dm,
                                                                        gulp=overlap + 16 * 8)]
        for k, ((delays, md, nout), s) in enumerate(zip(layout, plan.steps)):
            assert one[k].shape == (s.dms.size, nout)
            dc.assert_same_bits(small[k], one[k], f"step {k}: gulp")
            ref = dd.dedisperse_ds_host(raw, delays, md, s.downsamp, mask=mask, nout=nout, zero_dm=zero_dm, nbits=nbits)
            dc.assert_same_bits(one[k], ref, f"step {k}: the host specification on the whole file")
    if nbits is None:
        # the minimum: one decimated sample of the coarsest step above the overlap
        base = dd.dedisperse_filterbank_plan(fb, plan, mask=mask)
        least = dd.dedisperse_filterbank_plan(fb, plan, mask=mask, gulp=overlap + 16)
        for k in range(3):
            dc.assert_same_bits(least[k].cpu().numpy(), base[k].cpu().numpy(), f"step {k}: the least gulp")
    with pytest.raises(ValueError, match=f"gulp must be a multiple of 16 above the overlap of {overlap} samples"):
        dd.dedisperse_filterbank_plan(fb, plan, gulp=overlap + 15)
    with pytest.raises(ValueError, match="over the budget"):
        dd.dedisperse_filterbank_plan(fb, plan, budget_bytes=1 << 16)
    # a shard covers the same stretch: its rows are the whole plan's
    part = dd.dedisperse_filterbank_plan(fb, plan.shard(1, 2), mask=mask, zero_dm=True)
    for t, s in zip(part, plan.shard(1, 2).steps):
        k = [p.downsamp for p in plan.steps].index(s.downsamp)
        dc.assert_same_bits(t.cpu().numpy(), np.ascontiguousarray(one[k][1::2]), "shard")


def test_side_stream(torch):
    from riptide_amd import dedispersion as dd
    nsamp_blk, nchans = 16389, 70
    x, _, _ = _samples(21, nsamp_blk, nchans, "uint8", False)
    specs = []
    for f in (1, 3, 16):
        d = dp.delay_table(NDM, nchans, 40)
        specs.append((d, int(d.max()), f))
    side = torch.cuda.Stream()
    got, _, _ = run_steps(torch, x, None, specs, stream=side)
    for g, (d, md, f) in zip(got, specs):
        dc.assert_same_bits(g, dd.dedisperse_ds_host(x, d, md, f), f"f {f} on a side stream")


def test_refusals_launch_nothing(torch):
    from riptide_amd import engine
    nsamp_blk, nchans = 1000, 16
    x = np.full((nsamp_blk, nchans), 9, dtype=np.uint8)
    xd = _dev(torch, x)
    d = _dev(torch, np.zeros((3, nchans), dtype=np.int32))
    out = torch.full((3 * 1000,), -3.0, dtype=torch.float32, device="cuda")

    def step(**kw):
        base = dict(delays_off=0, out_off=0, out_stride=1000, out_offset=0, ndm=3, max_delay=10, downsamp=4,
                    reserved=0)
        base.update(kw)
        return np.array([tuple(base[n] for n in engine.DEDISP_STEP_DTYPE.names)], dtype=engine.DEDISP_STEP_DTYPE)

    bm = engine.DeviceBlockMask(_dev(torch, np.ones((30, nchans), dtype=np.uint8)),
                                _dev(torch, np.zeros(nchans, dtype=np.uint8)), 37)
    small = torch.empty(engine.dedisperse_steps_workspace_bytes("uint8", nsamp_blk, nchans, [4]) - 1,
                        dtype=torch.uint8, device="cuda")
    refused = [
        (dict(steps=step(downsamp=0)), r"downsamp 0 is outside \[1, 256\]"),
        (dict(steps=step(downsamp=257)), r"downsamp 257 is outside \[1, 256\]"),
        (dict(steps=step(max_delay=250)), "max_delay 250 is not below the 250 decimated samples"),
        (dict(steps=step(), block_mask=bm, t_origin=6), "t_origin 6 is not a multiple of downsamp 4"),
        (dict(steps=step(out_stride=200)), "out_stride is shorter than out_offset plus the step's outputs"),
        (dict(steps=step(delays_off=1)), "its delay table leaves the delay array"),
        (dict(steps=step(), workspace=small), "workspace must be a contiguous uint8 tensor of >= "),
    ]
    for kw, message in refused:
        with pytest.raises(ValueError, match=message):
            engine.dedisperse_steps_device(xd, d, out=out, **kw)
    # the exactness cap: 255 * 256 * 258 >= 2^24
    wide = _dev(torch, np.zeros((512, 258), dtype=np.uint8))
    with pytest.raises(ValueError, match="258 channels at downsamp 256 are too many for an exact sum"):
        engine.dedisperse_steps_device(wide, _dev(torch, np.zeros((1, 258), dtype=np.int32)),
                                       step(downsamp=256, ndm=1, max_delay=0), out)
    # the entry point's own workspace check, behind the wrapper's
    import ctypes
    from riptide_amd import _lib
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    st = step()
    rc = _lib.load().rt_dedisperse_steps_device(_lib.ptr(xd), 0, nsamp_blk, nchans, _lib.ptr(d), d.numel(), None,
                                                _lib.ptr(st), 1, _lib.ptr(out), out.numel(), _lib.ptr(ws),
                                                small.numel(), ctypes.c_void_p(0), 0, None)
    assert rc != 0 and "workspace too small" in _lib.load().rt_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())
    # and the accepted call writes
    engine.dedisperse_steps_device(xd, d, step(), out)
    assert float(out[0]) == 9.0 * 4 * nchans and float(out[240]) == -3.0


def test_end_to_end_search_of_a_decimated_trial(torch, tmp_path):
    import riptide_amd
    from riptide_amd.dispatch import EngineSearcher
    from riptide_amd.reading import Filterbank, write_sigproc
    plan = dp.e2e_plan()
    k, dm_true = dp.e2e_true_dm(plan)
    assert plan.downsamp[k] >= 4 and 1 in plan.downsamp
    fname = str(tmp_path / "pulsar.fil")
    write_sigproc(fname, dp.e2e_data(dm_true), dp.e2e_header())
    fb = Filterbank(fname)
    assert np.allclose(fb.freqs, dp.e2e_freqs())
    searcher = EngineSearcher(dp.E2E_DEREDDEN, dp.E2E_RANGES, device=0, batch=8)
    peaks = riptide_amd.search_filterbank_plan(fname, plan, searcher)
    assert len(peaks) > 0 and {p.dm for p in peaks} <= set(plan.dms.tolist())
    best = max(peaks, key=lambda p: p.snr)
    print("best", best, "true DM", dm_true, "trial", plan.dms[k])
    assert best.dm == plan.dms[k]
    # one trial step: at period P the FFA's period step is tau * P / T with a bin tau <= P / bins_min
    assert abs(best.period - dp.E2E["period"]) <= dp.e2e_period_step(), best
    # the searcher's lists are in plan order, and the f = 1 step is search_filterbank's, cut to the same length
    per = searcher.search_filterbank_plan(fb, plan)
    assert len(per) == len(plan) and [tuple(p) for plist in per for p in plist] == [tuple(p) for p in peaks]
    # a budget the plan does not fit at once: searched slice by slice, the same peaks
    from riptide_amd.dedispersion import plan_device_bytes, plan_layout, plan_slices
    budget = plan_device_bytes(fb, plan) * 9 // 10      # the gulp buffers and the workspace are most of it
    assert len(plan_slices(fb, plan, budget, chunk=8)) > 1
    sliced = searcher.search_filterbank_plan(fb, plan, budget_bytes=budget)
    assert [[tuple(p) for p in plist] for plist in sliced] == [[tuple(p) for p in plist] for plist in per]
    first = plan.steps[0]
    assert first.downsamp == 1
    nout = plan_layout(fb, plan)[0][2]
    ref = searcher.search_filterbank(fb, list(first.dms), nout=nout)
    assert [[tuple(p) for p in plist] for plist in per[:first.dms.size]] == [[tuple(p) for p in plist]
                                                                            for plist in ref]
    assert any(per[:first.dms.size])
