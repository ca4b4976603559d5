"""GPU tests of the block mask (csrc/dedisp_kernels.hip: the DdCells forms of
the transposes and of the row mean, the block statistics) and of what is built
on it.  The core assertion everywhere: the masked call on x equals, bit for
bit, the existing plain call on x' = rfi.apply_block_mask_host(x), both run on
the device.  The replacement itself and the statistics' host form are pinned to
numpy by test_blockmask_host.py."""
import numpy as np
import pytest

import blockmask_common as bc
import dedisp_common as dc
import rfi_common as rc

pytestmark = pytest.mark.gpu

DMS = [0.0, 3.0, 1.5]          # small delays: the sum kernel is unchanged
BLOCK_LENS = (1, 3, 64, 256, 300, 5000)
CASES = ([(f, n) for f in ("uint8", "int8", "float32") for n in (1, 3, 64, 65, 257)]
         + [(f, n) for f in ("u1", "u2", "u4") for n in (8, 520)] + [("u16", 3), ("u16", 65)]
         # rows of 12 bytes: the packed transposes' dword loads (8 and 520 one- and two-bit channels take byte loads)
         + [("u1", 96), ("u2", 48)])


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def _dev(torch, a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)       # the same bits
    return torch.from_numpy(a).cuda()


def _device_mask(torch, cells, fill, block_len):
    from riptide_amd import engine
    return engine.DeviceBlockMask(_dev(torch, np.asarray(cells, dtype=np.uint8)), _dev(torch, fill), block_len)


def _chan_mask(nchans):
    m = np.zeros(nchans, dtype=np.uint8)
    m[[0, nchans // 2]] = 1
    return m


def _delays(nchans):
    from riptide_amd.dedispersion import dispersion_delays
    return dispersion_delays(dc.band(nchans), DMS, dc.TSAMP)


def _combos(rng, nsamp_blk, nchans):
    """(block_len, t_origin, mask kind, cells, zero_dm, channel mask on): every
    block length with every t_origin, zero_dm x channel mask crossed, the six
    mask kinds rotating so each meets each of the four."""
    k = 0
    for block_len in BLOCK_LENS:
        for t_origin in sorted({0, 5, block_len - 1}):
            kinds = bc.mask_kinds(rng, bc.nblocks_for(nsamp_blk, block_len, t_origin), nchans)
            names = list(kinds)
            for zero_dm in (False, True):
                for cm in (False, True):
                    name = names[k % len(names)]
                    k += 1
                    yield block_len, t_origin, name, kinds[name], zero_dm, cm


@pytest.mark.parametrize("family,nchans", CASES)
def test_dedisperse_device_masked(torch, family, nchans):
    """dedisperse_device(block_mask=) on x against the plain call on x', bit
    for bit: blocks of 1 + max_delay, 255, 257 and 1000 rows, block lengths 1,
    3, 64, 256, 300 and one longer than the block, t_origin 0, 5 and
    block_len - 1 (a block boundary inside a tile and inside a wave's four
    rows of the row mean)."""
    from riptide_amd import engine, rfi
    nbits = bc.FAMILIES[family][1]
    delays, max_delay = _delays(nchans)
    d = _dev(torch, delays.astype(np.int32))
    rng = np.random.RandomState(nchans)
    fill = bc.fill_of(rng, family, nchans)
    cm_dev = _dev(torch, _chan_mask(nchans))
    for nsamp_blk in (1 + max_delay, 255, 257, 1000):
        x = bc.as_block(bc.values(rng, family, nsamp_blk, nchans), family)
        xd = _dev(torch, x)
        for block_len, t_origin, kind, cells, zero_dm, cm in _combos(rng, nsamp_blk, nchans):
            kw = dict(mask=cm_dev if cm else None, zero_dm=zero_dm, nbits=nbits)
            bm = _device_mask(torch, cells, fill, block_len)
            got = engine.dedisperse_device(xd, d, max_delay, block_mask=bm, t_origin=t_origin, **kw).cpu().numpy()
            xp = rfi.apply_block_mask_host(x, cells, block_len, fill, t_origin=t_origin, nbits=nbits)
            ref = engine.dedisperse_device(_dev(torch, xp), d, max_delay, **kw).cpu().numpy()
            assert got.shape == (len(DMS), nsamp_blk - max_delay)
            assert np.array_equal(got, ref), (nsamp_blk, block_len, t_origin, kind, zero_dm, cm)


@pytest.mark.parametrize("family,nchans", [("uint8", 65), ("int8", 65), ("float32", 65), ("u1", 72), ("u2", 68),
                                            ("u4", 66), ("u16", 65)])
def test_dedisperse_bands_device_masked(torch, family, nchans):
    """One case per sample family with an empty band, overlapping bands and the
    full band, with and without the zero-DM filter."""
    from riptide_amd import engine, rfi
    nbits = bc.FAMILIES[family][1]
    delays, max_delay = _delays(nchans)
    d = _dev(torch, delays.astype(np.int32))
    rng = np.random.RandomState(7)
    nsamp_blk, block_len, t_origin = 700, 64, 63
    x = bc.as_block(bc.values(rng, family, nsamp_blk, nchans), family)
    fill = bc.fill_of(rng, family, nchans)
    cells = rng.rand(bc.nblocks_for(nsamp_blk, block_len, t_origin), nchans) < 0.3
    bands = np.array([[5, 5], [0, 40], [20, nchans], [0, nchans]], dtype=np.uint32)
    bm = _device_mask(torch, cells, fill, block_len)
    xp = rfi.apply_block_mask_host(x, cells, block_len, fill, t_origin=t_origin, nbits=nbits)
    for zero_dm in (False, True):
        kw = dict(mask=_dev(torch, _chan_mask(nchans)), zero_dm=zero_dm, nbits=nbits)
        got = engine.dedisperse_bands_device(_dev(torch, x), d, max_delay, bands, block_mask=bm, t_origin=t_origin,
                                             **kw).cpu().numpy()
        ref = engine.dedisperse_bands_device(_dev(torch, xp), d, max_delay, bands, **kw).cpu().numpy()
        assert got.shape == (len(DMS), 4, nsamp_blk - max_delay) and np.array_equal(got, ref), zero_dm
        assert not got[:, 0].any()
        plain = engine.dedisperse_device(_dev(torch, x), d, max_delay, block_mask=bm, t_origin=t_origin, **kw)
        assert np.array_equal(got[:, 3], plain.cpu().numpy())


@pytest.mark.parametrize("family,nchans", CASES)
def test_zero_dm_mean_masked(torch, family, nchans):
    """zero_dm_mean_device(block_mask=) against the plain call on x', the same
    bits; for <= 8-bit data also rfi_common.numpy_zero_dm_mean(x')."""
    from riptide_amd import engine, rfi
    nbits = bc.FAMILIES[family][1]
    rng = np.random.RandomState(100 + nchans)
    fill = bc.fill_of(rng, family, nchans)
    for nsamp_blk in (1, 255, 1000):
        x = bc.as_block(bc.values(rng, family, nsamp_blk, nchans), family)
        xd = _dev(torch, x)
        for block_len, t_origin, kind, cells, _, cm in _combos(rng, nsamp_blk, nchans):
            mask = _chan_mask(nchans) if cm and nchans > 2 else None
            bm = _device_mask(torch, cells, fill, block_len)
            got = engine.zero_dm_mean_device(xd, mask=_dev(torch, mask), nbits=nbits, block_mask=bm,
                                             t_origin=t_origin).cpu().numpy()
            xp = rfi.apply_block_mask_host(x, cells, block_len, fill, t_origin=t_origin, nbits=nbits)
            ref = engine.zero_dm_mean_device(_dev(torch, xp), mask=_dev(torch, mask), nbits=nbits).cpu().numpy()
            assert np.array_equal(got, ref), (nsamp_blk, block_len, t_origin, kind, cm)
            if family != "float32" and nbits != 16:
                assert np.array_equal(got, rc.numpy_zero_dm_mean(bc.as_values(xp, family, nchans), mask))


@pytest.mark.parametrize("nchans", [1, 65])
@pytest.mark.parametrize("family", list(bc.FAMILIES))
def test_block_stats_device(torch, family, nchans):
    """block_stats_device against rt_block_stats_host, bit for bit for every
    sample type, at the host test's shapes; twice the same bits."""
    from riptide_amd import _lib, engine
    lib = _lib.load()
    nbits = bc.FAMILIES[family][1]
    nsamp = 6000
    nchans = bc.whole_bytes(family, nchans)
    x = bc.as_block(bc.values(np.random.RandomState(nchans), family, nsamp, nchans), family)
    xd = _dev(torch, x)
    for block_len in (1, 5, 2048, 2049, 5000, 10 * nsamp):
        nblk = -(-nsamp // block_len)
        ref = np.zeros((nblk, 2, nchans))
        assert lib.rt_block_stats_host(_lib.ptr(x), bc.DTYPE_CODES[family], nsamp, nchans, block_len,
                                       _lib.ptr(ref)) == _lib.RT_OK
        out = torch.full((nblk, 2, nchans), -7.0, dtype=torch.float64, device="cuda")    # written, not accumulated
        got = engine.block_stats_device(xd, block_len, out=out, nbits=nbits)
        assert got is out and np.array_equal(out.cpu().numpy(), ref), block_len
        assert np.array_equal(engine.block_stats_device(xd, block_len, nbits=nbits).cpu().numpy(), ref)
    with pytest.raises(ValueError, match="block_len"):
        engine.block_stats_device(xd, 0, nbits=nbits)
    with pytest.raises(ValueError, match="out must be"):
        engine.block_stats_device(xd, 2048, out=out, nbits=nbits)


def _write_filterbank(path, x):
    from riptide_amd.reading import write_sigproc
    nchans = x.shape[1]
    header = {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": dc.TSAMP,
              "nbits": 8 * x.dtype.itemsize, "fch1": 400.0, "foff": -32.0 / nchans, "nchans": nchans, "nifs": 1}
    write_sigproc(str(path), x, header)
    return str(path)


FILE_DMS = [0.0, 50.0, 12.5]


@pytest.mark.parametrize("name", ["uint8", "float32"])
def test_filterbank_gulps(torch, tmp_path, name):
    """dedisperse_filterbank(block_mask=) with block_len 100 at gulps of
    max_delay + 1, 333 and the whole file: identical bits, those of the plain
    call on a file holding x', with the channel mask and the zero-DM filter
    too; rfi.block_stats and zero_dm_series do not depend on gulp."""
    from riptide_amd import _lib, rfi
    from riptide_amd.dedispersion import dedisperse_filterbank, dispersion_delays
    from riptide_amd.reading import Filterbank
    nchans = 32
    _, max_delay = dispersion_delays(dc.band(nchans), FILE_DMS, dc.TSAMP)
    rng = np.random.RandomState(11)
    x = dc.samples(rng, 4096 + max_delay, nchans, np.dtype(name))
    fb = Filterbank(_write_filterbank(tmp_path / "x.fil", x))
    nblocks = -(-x.shape[0] // 100)
    bm = rfi.BlockMask(rng.rand(nblocks, nchans) < 0.3, 100, rng.normal(3.0, 40.0, size=nchans))
    xp = rfi.apply_block_mask_host(x, bm.cells, 100, bm.typed_fill(fb))
    fbp = Filterbank(_write_filterbank(tmp_path / "xp.fil", xp))
    cmask = np.zeros(nchans, dtype=bool)
    cmask[5] = True
    for kw in ({}, {"zero_dm": True, "mask": cmask}):
        ref = dedisperse_filterbank(fbp, FILE_DMS, **kw).cpu().numpy()
        for gulp in (max_delay + 1, 333, None):
            out = dedisperse_filterbank(fb, FILE_DMS, gulp=gulp, block_mask=bm, **kw)
            assert out.is_cuda and np.array_equal(out.cpu().numpy(), ref), (gulp, kw)
        assert not np.array_equal(dedisperse_filterbank(fb, FILE_DMS, **kw).cpu().numpy(), ref)
    series = rfi.zero_dm_series(fbp, mask=cmask).cpu().numpy()
    for gulp in (333, None):
        assert np.array_equal(rfi.zero_dm_series(fb, mask=cmask, gulp=gulp, block_mask=bm).cpu().numpy(), series)
    # the statistics: every gulp the bits of the host specification
    lib = _lib.load()
    host = np.zeros((nblocks, 2, nchans))
    assert lib.rt_block_stats_host(_lib.ptr(x), 0 if name == "uint8" else 2, x.shape[0], nchans, 100,
                                   _lib.ptr(host)) == _lib.RT_OK
    for gulp in (100, 333, None):
        st = rfi.block_stats(fb, block_len=100, gulp=gulp)
        assert st.block_len == 100 and st.nsamp == x.shape[0] and st.count[-1] == x.shape[0] - (nblocks - 1) * 100
        assert np.array_equal(st.sum, host[:, 0]) and np.array_equal(st.sumsq, host[:, 1]), gulp
    part = rfi.block_stats(fb, block_len=100, nsamp=250, gulp=100)      # a partial last block
    host3 = np.zeros((3, 2, nchans))
    assert lib.rt_block_stats_host(_lib.ptr(x), 0 if name == "uint8" else 2, 250, nchans, 100,
                                   _lib.ptr(host3)) == _lib.RT_OK
    assert part.count.tolist() == [100, 100, 50] and np.array_equal(part.sum, host3[:, 0])
    assert np.array_equal(part.sumsq, host3[:, 1])
    # refusals of the file calls
    with pytest.raises(ValueError, match="channels"):
        dedisperse_filterbank(fb, FILE_DMS, block_mask=rfi.BlockMask(bm.cells[:, :31], 100, bm.fill[:31]))
    with pytest.raises(ValueError, match="fewer than"):
        dedisperse_filterbank(fb, FILE_DMS, block_mask=rfi.BlockMask(bm.cells[:-1], 100, bm.fill))
    ndm, nout = len(FILE_DMS), x.shape[0] - max_delay
    if name == "uint8":      # the budget counts the cells and the fill
        budget = ndm * nout * 4 + 2 * 333 * nchans + 336 * nchans
        dedisperse_filterbank(fb, FILE_DMS, gulp=333, budget_bytes=budget)
        with pytest.raises(ValueError, match="pass fewer DMs per call"):
            dedisperse_filterbank(fb, FILE_DMS, gulp=333, budget_bytes=budget + nblocks * nchans, block_mask=bm)
        dedisperse_filterbank(fb, FILE_DMS, gulp=333, budget_bytes=budget + (nblocks + 1) * nchans, block_mask=bm)
    with pytest.raises(ValueError, match="use longer blocks"):
        rfi.block_stats(fb, block_len=100, budget_bytes=nblocks * 2 * nchans * 8)


def _write_packed(path, packed, nbits, nchans):
    """Packed rows uint8 [nsamp, row_bytes] -> a SIGPROC file of that width."""
    from riptide_amd.reading import write_sigproc
    header = {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": dc.TSAMP,
              "nbits": nbits, "fch1": 400.0, "foff": -32.0 / nchans, "nchans": nchans, "nifs": 1}
    write_sigproc(str(path), np.ascontiguousarray(packed).ravel(), header)
    return str(path)


@pytest.mark.parametrize("nbits", [1, 2, 16])
def test_packed_filterbank_masked(torch, tmp_path, nbits):
    """The file calls on a PackedFilterbank with a block mask -- the typed
    fill (uint8, or uint16 for 16-bit data) and its upload: the band form of
    dedisperse_filterbank, zero_dm_series and block_stats against the plain
    calls on a file holding x' and the host statistics."""
    from riptide_amd import _lib, rfi
    from riptide_amd.dedispersion import dedisperse_filterbank, dispersion_delays
    from riptide_amd.reading import PackedFilterbank, open_filterbank, pack_samples
    nchans, family = 32, f"u{nbits}"
    _, max_delay = dispersion_delays(dc.band(nchans), FILE_DMS, dc.TSAMP)
    rng = np.random.RandomState(nbits)
    nsamp = 1500 + max_delay
    packed = pack_samples(bc.values(rng, family, nsamp, nchans), nbits)
    fb = open_filterbank(_write_packed(tmp_path / "p.fil", packed, nbits, nchans))
    assert isinstance(fb, PackedFilterbank)
    nblocks = -(-nsamp // 100)
    bm = rfi.BlockMask(rng.rand(nblocks, nchans) < 0.3, 100, rng.uniform(-2.0, (1 << nbits) + 1.0, size=nchans))
    fill = bm.typed_fill(fb)
    assert fill.dtype == (np.uint16 if nbits == 16 else np.uint8) and fill.max() <= (1 << nbits) - 1
    xp = rfi.apply_block_mask_host(packed, bm.cells, 100, fill, nbits=nbits)
    assert not np.array_equal(xp, packed)
    fbp = open_filterbank(_write_packed(tmp_path / "pp.fil", xp, nbits, nchans))
    bands = np.array([[0, 8], [4, 32], [9, 9], [0, 32]], dtype=np.uint32)
    for kw in ({}, {"zero_dm": True}):
        ref = dedisperse_filterbank(fbp, FILE_DMS, bands=bands, **kw).cpu().numpy()
        for gulp in (333, None):
            got = dedisperse_filterbank(fb, FILE_DMS, bands=bands, gulp=gulp, block_mask=bm, **kw).cpu().numpy()
            assert got.shape == (len(FILE_DMS), 4, 1500) and np.array_equal(got, ref), (gulp, kw)
        assert np.array_equal(dedisperse_filterbank(fb, FILE_DMS, block_mask=bm, **kw).cpu().numpy(), ref[:, 3])
    series = rfi.zero_dm_series(fbp).cpu().numpy()
    assert np.array_equal(rfi.zero_dm_series(fb, gulp=333, block_mask=bm).cpu().numpy(), series)
    assert not np.array_equal(rfi.zero_dm_series(fb).cpu().numpy(), series)
    host = np.zeros((nblocks, 2, nchans))
    assert _lib.load().rt_block_stats_host(_lib.ptr(packed), bc.DTYPE_CODES[family], nsamp, nchans, 100,
                                           _lib.ptr(host)) == _lib.RT_OK
    for gulp in (333, None):
        st = rfi.block_stats(fb, block_len=100, gulp=gulp)
        assert np.array_equal(st.sum, host[:, 0]) and np.array_equal(st.sumsq, host[:, 1]), gulp
    with pytest.raises(ValueError, match="block_len"):
        rfi.block_stats(fb, block_len=0)


def test_band_series_and_candidates_masked(torch, tmp_path):
    """block_mask= through band_series and build_candidates_filterbank: the
    series and the folds of the plain calls on a file holding x'."""
    import pandas  # noqa: F401  (Candidate.peaks is a DataFrame)
    from riptide_amd import Peak, PeakCluster, build_candidates_filterbank, rfi
    from riptide_amd.dedispersion import band_edges, band_series, dispersion_delays
    from riptide_amd.reading import Filterbank
    nchans, nsamp, period, dm = 32, 8192, 0.5, 20.0
    rng = np.random.RandomState(1234)
    x = rng.normal(100.0, 10.0, size=(nsamp, nchans))
    sweep = dc.numpy_delays(dc.band(nchans), [dm], dc.TSAMP)[0]
    for c in range(nchans):
        for t0 in range(100 + int(sweep[c]), nsamp - 8, 500):
            x[t0:t0 + 8, c] += 12.0
    x = np.clip(np.round(x), 0, 255).astype(np.uint8)
    fb = Filterbank(_write_filterbank(tmp_path / "c.fil", x))
    bm = rfi.BlockMask(rng.rand(32, nchans) < 0.2, 256, np.full(nchans, 100.0))
    xp = rfi.apply_block_mask_host(x, bm.cells, 256, bm.typed_fill(fb))
    fbp = Filterbank(_write_filterbank(tmp_path / "cp.fil", xp))
    dms = [dm, 0.0]
    _, max_delay = dispersion_delays(fb.freqs, dms, fb.tsamp)
    nout = nsamp - max_delay
    bands = np.concatenate([band_edges(nchans, 4), np.array([[0, nchans]], dtype=np.uint32)])
    mask = np.zeros(nchans, dtype=bool)
    mask[3] = True
    for kw in ({}, {"zero_dm": True, "mask": mask}):
        got, empty = band_series(fb, dms, bands, E2E_DEREDDEN, nout, block_mask=bm, **kw)
        ref, empty_ref = band_series(fbp, dms, bands, E2E_DEREDDEN, nout, **kw)
        assert np.array_equal(got.cpu().numpy(), ref.cpu().numpy()) and np.array_equal(empty, empty_ref)
        assert not np.array_equal(band_series(fb, dms, bands, E2E_DEREDDEN, nout, **kw)[0].cpu().numpy(),
                                  ref.cpu().numpy())
    ranges = [{"name": "short",
               "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
               "candidates": {"bins": 64, "subints": 4}}]
    clusters = [PeakCluster([Peak(period=period, freq=1.0 / period, width=3, ducy=3 / 64, iw=1, ip=0, snr=30.0,
                                  dm=dm)], rank=0)]
    got = build_candidates_filterbank(clusters, fb, ranges, E2E_DEREDDEN, nsub=4, block_mask=bm)
    ref = build_candidates_filterbank(clusters, fbp, ranges, E2E_DEREDDEN, nsub=4)
    plain = build_candidates_filterbank(clusters, fb, ranges, E2E_DEREDDEN, nsub=4)
    assert len(got) == len(ref) == 1
    assert np.array_equal(got[0].subints, ref[0].subints) and np.array_equal(got[0].subbands, ref[0].subbands)
    assert not np.array_equal(plain[0].subbands, ref[0].subbands)


def test_refusals(torch):
    """Rows past the mask, a wrong fill dtype and block_len = 0: ValueError,
    and nothing is launched -- the output keeps its sentinel."""
    from riptide_amd import engine
    nchans, nsamp_blk = 16, 300
    delays, max_delay = _delays(nchans)
    d = _dev(torch, delays.astype(np.int32))
    x = _dev(torch, dc.samples(np.random.RandomState(1), nsamp_blk, nchans, np.uint8))
    cells = torch.ones((3, nchans), dtype=torch.uint8, device="cuda")
    fill = torch.zeros(nchans, dtype=torch.uint8, device="cuda")
    out = torch.full((len(DMS), nsamp_blk - max_delay), -1.0, dtype=torch.float32, device="cuda")
    m = torch.full((nsamp_blk,), -1.0, dtype=torch.float32, device="cuda")

    def both(bm, t_origin, match):
        with pytest.raises(ValueError, match=match):
            engine.dedisperse_device(x, d, max_delay, out=out, block_mask=bm, t_origin=t_origin)
        with pytest.raises(ValueError, match=match):
            engine.dedisperse_bands_device(x, d, max_delay, np.array([[0, nchans]]), block_mask=bm, t_origin=t_origin)
        with pytest.raises(ValueError, match=match):
            engine.zero_dm_mean_device(x, out=m, block_mask=bm, t_origin=t_origin)

    engine.dedisperse_device(x, d, max_delay, block_mask=engine.DeviceBlockMask(cells, fill, 100))   # 300 rows fit
    both(engine.DeviceBlockMask(cells, fill, 100), 1, "reach past the mask")
    both(engine.DeviceBlockMask(cells[:2], fill, 100), 0, "reach past the mask")
    both(engine.DeviceBlockMask(cells, fill.to(torch.int8), 100), 0, "block_mask.fill must be")
    both(engine.DeviceBlockMask(cells, fill.to(torch.float32), 100), 0, "block_mask.fill must be")
    both(engine.DeviceBlockMask(cells, fill[:15], 100), 0, "block_mask.fill must be")
    both(engine.DeviceBlockMask(cells, fill, 0), 0, "block_len")
    both(engine.DeviceBlockMask(cells[:, :15], fill, 100), 0, "block_mask.cells must be")
    both(engine.DeviceBlockMask(cells.cpu(), fill, 100), 0, "block_mask.cells must be")
    both(engine.DeviceBlockMask(cells, fill, 100), -1, "t_origin")
    both(engine.DeviceBlockMask(cells, fill, 100), 1 << 64, "t_origin")              # not truncated to 0
    both(engine.DeviceBlockMask(cells[:1], fill, (1 << 64) - 1), (1 << 64) - 100, "overflows 64 bits")
    # a band table of no rows: refused with a block mask as without one, never the plain call's writes
    bout = torch.full((len(DMS), 2, nsamp_blk - max_delay), -1.0, dtype=torch.float32, device="cuda")
    none = np.zeros((0, 2), dtype=np.uint32)
    with pytest.raises(ValueError, match="nbands must be at least 1"):
        engine.dedisperse_bands_device(x, d, max_delay, none, out=bout[:, :0])
    with pytest.raises(ValueError, match="nbands must be at least 1"):
        engine.dedisperse_bands_device(x, d, max_delay, none, out=bout[:, :0],
                                       block_mask=engine.DeviceBlockMask(cells, fill, 100))
    torch.cuda.synchronize()
    assert bool((bout == -1.0).all())
    xf = x.to(torch.float32)
    with pytest.raises(ValueError, match="block_mask.fill must be"):
        engine.dedisperse_device(xf, d, max_delay, block_mask=engine.DeviceBlockMask(cells, fill, 100))
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((m == -1.0).all())


def test_plain_calls_unchanged(torch):
    """With block_mask=None each entry point returns the bits it returns
    today: the exact sums of the host specification, the row mean of the
    numpy restatement, and the _cells entry point with a NULL mask gives the
    array of the old one."""
    import ctypes
    from riptide_amd import _lib, engine
    lib = _lib.load()
    nchans, nout = 65, 500
    delays, max_delay = _delays(nchans)
    d = _dev(torch, delays.astype(np.int32))
    bands = np.array([[0, 16], [10, 65], [0, 65]], dtype=np.uint32)
    for dtype in (np.uint8, np.int8, np.float32):
        x = dc.samples(np.random.RandomState(2), max_delay + nout, nchans, dtype)
        block = _dev(torch, x)
        out = engine.dedisperse_device(block, d, max_delay, block_mask=None).cpu().numpy()
        dc.assert_dedispersed(out, x, delays, nout)
        assert np.array_equal(out, engine.dedisperse_device(block, d, max_delay).cpu().numpy())
        b = engine.dedisperse_bands_device(block, d, max_delay, bands, block_mask=None).cpu().numpy()
        assert np.array_equal(b[:, 2], out)
        for i, (lo, hi) in enumerate(bands[:2]):
            keep = np.ones(nchans, dtype=bool)
            keep[lo:hi] = False
            dc.assert_dedispersed(b[:, i], x, delays, nout, keep)
        m = engine.zero_dm_mean_device(block, block_mask=None).cpu().numpy()
        if dtype == np.float32:
            ref = rc.numpy_zero_dm_mean(x)
            assert np.all(np.abs(m.astype(np.float64) - ref) <= 2.0 ** -23 * np.abs(ref))
        else:
            assert np.array_equal(m, rc.numpy_zero_dm_mean(x))
        ws = torch.empty(engine.dedisperse_workspace_bytes(np.dtype(dtype).name, x.shape[0], nchans), dtype=torch.uint8,
                         device="cuda")
        raw = torch.empty((len(DMS), nout), dtype=torch.float32, device="cuda")
        assert lib.rt_dedisperse_device_cells(_lib.ptr(block), engine.DEDISP_DTYPES[np.dtype(dtype).name], x.shape[0],
                                              nchans, _lib.ptr(d), None, len(DMS), None, 0, max_delay, _lib.ptr(raw),
                                              nout, 0, _lib.ptr(ws), ws.numel(), engine._stream_handle(), 0,
                                              None) == _lib.RT_OK
        assert np.array_equal(raw.cpu().numpy(), out)
        # a mask that flags nothing is the plain call too
        none = engine.DeviceBlockMask(torch.zeros((1, nchans), dtype=torch.uint8, device="cuda"),
                                      _dev(torch, np.zeros(nchans, dtype=dtype)), x.shape[0])
        assert np.array_equal(engine.dedisperse_device(block, d, max_delay, block_mask=none).cpu().numpy(), out)
        bm = _lib.BlockMaskStruct(none.cells.data_ptr(), 1, 0, 0, none.fill.data_ptr())
        assert lib.rt_zero_dm_mean_device_cells(_lib.ptr(block), engine.DEDISP_DTYPES[np.dtype(dtype).name],
                                                x.shape[0], nchans, None, _lib.ptr(raw), engine._stream_handle(),
                                                ctypes.byref(bm)) == _lib.RT_EINVAL      # block_len == 0


# ---------------------------------------------------------------- end to end
E2E_DMS = [0.0, 30.0]
E2E_DM, E2E_PERIOD, E2E_RFI_PERIOD = 30.0, 0.25, 0.4
E2E_CHANS, E2E_BLOCKS = slice(12, 16), slice(10, 15)
E2E_DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}
E2E_RANGES = [{"name": "short",
               "ffa_search": {"period_min": 0.09, "period_max": 1.0, "bins_min": 80, "bins_max": 88},
               "find_peaks": {"smin": 7.0}}]
E2E_BURST = 12 * 2048 + 1100


def _e2e_samples(burst=False):
    """32 channels x 2^16 samples of 1 ms, noise N(100, 10): a train of
    8-sample pulses of amplitude 3 and period 0.25 s swept at DM 30; in
    channels 12-15, during blocks 10-14 of 2048 samples (5 of 32), undispersed
    pulses of amplitude 30, period 0.4 s and 40 samples; with `burst` one more
    40-sample burst of amplitude 60 in those channels, off that train."""
    nchans, nsamp = 32, 1 << 16
    rng = np.random.RandomState(2468)
    x = rng.normal(100.0, 10.0, size=(nsamp, nchans))
    sweep = dc.numpy_delays(dc.band(nchans), [E2E_DM], dc.TSAMP)[0]
    for c in range(nchans):
        for t0 in range(100 + int(sweep[c]), nsamp - 8, 250):
            x[t0:t0 + 8, c] += 3.0
    t = np.arange(nsamp)
    on = (t >= E2E_BLOCKS.start * 2048) & (t < E2E_BLOCKS.stop * 2048) & ((t % 400) < 40)
    x[on, E2E_CHANS] += 30.0
    if burst:
        x[E2E_BURST:E2E_BURST + 40, E2E_CHANS] += 60.0
    return np.clip(np.round(x), 0, 255).astype(np.uint8)


def _near(period, target):
    return abs(period - target) <= 0.01 * target


def test_end_to_end(torch, tmp_path):
    """Block statistics -> block mask -> search, without the zero-DM filter.
    The amplitudes were fixed on the CPU through apply_block_mask_host,
    dedisperse_host and the oracle's periodogram (dereddened and normalised
    as the searcher does), largest S/N over the widths:

      unmasked  DM 0: 22.9 at 0.4 s, the top peak (7.2 near 0.25 s)
                DM 30: 65.6 at 0.25 s (22.0 near 0.4 s)
      masked    DM 0: 4.5 near 0.4 s, 6.6 at most anywhere
                DM 30: 66.5 at 0.25 s, the top peak (9.1 near 0.4 s)
    """
    from riptide_amd import rfi
    from riptide_amd.dispatch import EngineSearcher, search_filterbank
    from riptide_amd.reading import Filterbank
    x = _e2e_samples()
    fb = Filterbank(_write_filterbank(tmp_path / "e2e.fil", x))
    searcher = EngineSearcher(E2E_DEREDDEN, E2E_RANGES, device=0, batch=2)

    plain = search_filterbank(fb, E2E_DMS, searcher)
    dm0 = [p for p in plain if p.dm == 0.0]
    assert dm0 and _near(max(dm0, key=lambda p: p.snr).period, E2E_RFI_PERIOD)
    pulsar_plain = max(p.snr for p in plain if p.dm == E2E_DM and _near(p.period, E2E_PERIOD))

    bm = rfi.block_mask(rfi.block_stats(fb))
    assert bm.block_len == 2048 and bm.cells.shape == (32, 32)
    assert bm.cells[E2E_BLOCKS, E2E_CHANS].all()                      # 1. the run is covered
    assert bm.fraction < 0.03 and not bm.channel_mask().any()
    clean = search_filterbank(fb, E2E_DMS, searcher, block_mask=bm)
    at_dm = [p for p in clean if p.dm == E2E_DM]
    top = max(at_dm, key=lambda p: p.snr)
    rfi_left = max([p.snr for p in clean if p.dm == 0.0 and _near(p.period, E2E_RFI_PERIOD)], default=0.0)
    assert rfi_left < top.snr                                         # 2. the interference is below the pulsar
    assert _near(top.period, E2E_PERIOD) and top.snr >= pulsar_plain  # 3. the pulsar on top, no weaker
    assert max(p.snr for p in clean) == top.snr
    # the masked search is the plain search of a file holding x'
    xp = rfi.apply_block_mask_host(x, bm.cells, bm.block_len, bm.typed_fill(fb))
    fbp = Filterbank(_write_filterbank(tmp_path / "e2e_replaced.fil", xp))
    assert [tuple(p) for p in search_filterbank(fbp, E2E_DMS, searcher)] == [tuple(p) for p in clean]


def test_search_filterbank_pulses_masked(torch, tmp_path):
    """A 40-sample burst confined to the flagged cells: a SinglePulse
    unmasked, none masked."""
    from riptide_amd import rfi
    from riptide_amd.reading import Filterbank
    from riptide_amd.single_pulse import search_filterbank_pulses
    fb = Filterbank(_write_filterbank(tmp_path / "burst.fil", _e2e_samples(burst=True)))
    bm = rfi.block_mask(rfi.block_stats(fb))
    assert bm.cells[E2E_BLOCKS, E2E_CHANS].all()

    def near_burst(pulses):
        return [p for p in pulses if abs(int(p.sample) - E2E_BURST) <= 100]

    plain, _ = search_filterbank_pulses(fb, [0.0], E2E_DEREDDEN, threshold=8.0)
    assert near_burst(plain)
    masked, _ = search_filterbank_pulses(fb, [0.0], E2E_DEREDDEN, threshold=8.0, block_mask=bm)
    assert not near_burst(masked) and not masked
    # the same through dispatch.search_filterbank(pulses=), the searcher's combined path
    from riptide_amd.dispatch import EngineSearcher, search_filterbank
    searcher = EngineSearcher(E2E_DEREDDEN, E2E_RANGES, device=0, batch=2)
    peaks, found = search_filterbank(fb, E2E_DMS, searcher, pulses={"threshold": 8.0})
    assert near_burst([p for p in found if p.dm == 0.0])
    mpeaks, mfound = search_filterbank(fb, E2E_DMS, searcher, pulses={"threshold": 8.0}, block_mask=bm)
    assert not near_burst(mfound)
    assert [tuple(p) for p in mpeaks] == [tuple(p) for p in search_filterbank(fb, E2E_DMS, searcher, block_mask=bm)]
    assert [tuple(p) for p in mpeaks] != [tuple(p) for p in peaks]
