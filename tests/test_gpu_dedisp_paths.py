"""GPU tests that pin dedisp_sum_kernel (csrc/dedisp_kernels.hip) at every
staging path, byte residue and edge, with the hand-made integer delay tables of
dedisp_common (their preconditions: test_dedisp_host.py::test_path_tables).
The path of every (DM tile, channel) is named in the test by
engine.dedisperse_span_plan, the kernel's own rule.  Every comparison is bit
for bit, on uint32 views: integer sums against the exact float64 numpy sum
cast once and the host specification, float32 sums against
dc.numpy_dedisperse_f32 and the host specification.  No tolerance."""
import numpy as np
import pytest

import dedisp_common as dc
from test_dedisp_host import BAND_TABLE

pytestmark = pytest.mark.gpu

NOUT = 300      # one full time tile of 256 outputs and a partial one
ESIZE = {"uint8": 1, "int8": 1, "u1": 1, "u2": 1, "u4": 1, "float32": 4, "u16": 4}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


def run(torch, x, delays, max_delay, mask=None, bands=None, **kw):
    """engine.dedisperse_device, or with bands dedisperse_bands_device, on the
    whole of x as one block -> numpy."""
    from riptide_amd import engine
    block = torch.from_numpy(x).cuda()
    d = torch.from_numpy(np.asarray(delays).astype(np.int32)).cuda()
    m = None if mask is None else torch.from_numpy(np.asarray(mask, dtype=np.uint8)).cuda()
    if bands is None:
        return engine.dedisperse_device(block, d, max_delay, mask=m, **kw).cpu().numpy()
    return engine.dedisperse_bands_device(block, d, max_delay, bands, mask=m, **kw).cpu().numpy()


def exact_sums(vals, delays, nout, mask=None, bands=None):
    """Integer samples: the exact float64 sums, cast once."""
    if bands is None:
        return dc.numpy_dedisperse(vals, delays, nout, mask)[0].astype(np.float32)
    rows = []
    for lo, hi in bands:
        m = np.ones(vals.shape[1], dtype=bool)
        m[int(lo):int(hi)] = False
        if mask is not None:
            m |= np.asarray(mask, dtype=bool)
        rows.append(dc.numpy_dedisperse(vals, delays, nout, m)[0].astype(np.float32))
    return np.stack(rows, axis=1)


def check(torch, kind, delays, max_delay, mask=None, bands=None, zero_dm=False, seed=0, nout=NOUT):
    """One device call of seeded samples against both references; returns the
    device result."""
    from riptide_amd.dedispersion import dedisperse_bands_host, dedisperse_host
    x, vals, nbits = dc.kind_samples(np.random.RandomState(seed), max_delay + nout, delays.shape[1], kind)
    out = run(torch, x, delays, max_delay, mask, bands, zero_dm=zero_dm, nbits=nbits)
    if zero_dm or ESIZE[kind] == 4:
        mean = dc.numpy_zero_dm_mean(vals, mask) if zero_dm else None
        ref = dc.numpy_dedisperse_f32(vals, delays, nout, mask, bands=bands, mean=mean)
    else:
        ref = exact_sums(vals, delays, nout, mask, bands)
    dc.assert_same_bits(out, ref, f"{kind}: device against numpy")
    if bands is None:
        host = dedisperse_host(x, delays, max_delay, mask=mask, nout=nout, zero_dm=zero_dm, nbits=nbits)
    else:
        host = dedisperse_bands_host(x, delays, max_delay, bands, mask=mask, nout=nout, zero_dm=zero_dm, nbits=nbits)
    dc.assert_same_bits(out, host, f"{kind}: device against the host specification")
    return out


@pytest.mark.parametrize("r", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["uint8", "int8", "float32"])
def test_staging_threshold(torch, kind, r):
    """Channels exactly at the last staged span (ndw == 264 dwords of bytes,
    520 of floats: the aligned read reaches the span's spare dword), channels
    one sample beyond it (direct) and masked channels in one 16-channel step,
    both paths again in the partial step of four, at every lo % 4; 16 DMs, 17
    (a second DM tile of one DM and 15 repeated rows) and 5 (11 repeated
    rows)."""
    esize = ESIZE[kind]
    for ndm in (16, 17, 5):
        delays, mask, max_delay = dc.threshold_table(esize, r, ndm)
        paths = dc.tile_paths(delays, max_delay, esize, mask)
        assert {"S", "D", "M"} <= set(paths[0, :16]) and {"S", "D"} <= set(paths[0, 16:])
        assert paths.shape[0] == (2 if ndm == 17 else 1)
        check(torch, kind, delays, max_delay, mask, seed=10 * r + ndm)
        if ndm == 17:     # without the mask: 20 channels summed, the class M ones direct
            assert "M" not in dc.tile_paths(delays, max_delay, esize)
            check(torch, kind, delays, max_delay, seed=r)


@pytest.mark.parametrize("kind", ["uint8", "int8", "u4", "u2"])
def test_every_residue(torch, kind):
    """delay = lo_c + d, d = 0 .. 15: every rounding lo % 4 of the staged base
    with every byte residue p % 4 of the aligned read, all channels staged; 20
    channels (a full step and a partial one) and 32 (two full steps)."""
    for nchans in (20, 32):
        delays, max_delay = dc.residue_table(nchans)
        assert set(dc.tile_paths(delays, max_delay, 1).ravel()) == {"S"}
        check(torch, kind, delays, max_delay, seed=nchans)


def test_mixed_step_bias_and_bands(torch):
    """int8, where a channel count that is off by k shows as k * 128: staged,
    direct and masked channels in one step, through the band call.  Band 5,
    [11, 13), holds a direct and a masked channel alone; band 4 is empty; the
    row of [0, 20) has the plain call's bits."""
    for r, ndm in ((1, 17), (2, 5)):
        delays, mask, max_delay = dc.threshold_table(1, r, ndm)
        paths = dc.tile_paths(delays, max_delay, 1, mask)
        assert {"S", "D", "M"} <= set(paths[0, :16])
        assert set(paths[0, 11:13]) == {"D", "M"} and set(paths[0, 15:17]) == {"S"}
        out = check(torch, "int8", delays, max_delay, mask, bands=BAND_TABLE, seed=ndm)
        plain = check(torch, "int8", delays, max_delay, mask, seed=ndm)
        dc.assert_same_bits(out[:, 0], plain, "the band [0, 20) against the plain call")
        assert not out[:, 4].any() and out[:, 5].any()
        # no mask: every class M channel is summed too, on the direct path
        check(torch, "int8", delays, max_delay, bands=BAND_TABLE, seed=ndm + 1)


def test_saturated_partial_sums(torch):
    """32 channels of the largest and smallest samples, two full steps: the
    packed 16-bit partial sums hold 16 x 255 per field, and every output is
    32 * v exactly -- staged at every byte residue, then on the direct path."""
    rdel, rmax = dc.residue_table(32)
    tdel, _, tmax = dc.threshold_table(1, 1, 16, nchans=32)
    assert set(dc.tile_paths(rdel, rmax, 1).ravel()) == {"S"}
    assert (dc.tile_paths(tdel, tmax, 1) == "D").sum() >= 16
    for dtype, v in ((np.uint8, 255), (np.int8, 127), (np.int8, -128)):
        for delays, max_delay in ((rdel, rmax), (tdel, tmax)):
            x = np.full((max_delay + NOUT, 32), v, dtype=dtype)
            out = run(torch, x, delays, max_delay)
            assert out.shape == (delays.shape[0], NOUT)
            dc.assert_same_bits(out, np.full(out.shape, 32 * v, dtype=np.float32), f"{dtype.__name__} {v}")


@pytest.mark.parametrize("direct", [False, True], ids=["staged", "direct"])
@pytest.mark.parametrize("kind,rem", [("uint8", 0), ("uint8", 1), ("uint8", 15), ("int8", 15), ("float32", 0),
                                      ("float32", 1), ("float32", 3)])
def test_block_end(torch, kind, rem, direct):
    """One DM at max_delay in every channel: its last output reads row
    nsamp_blk - 1, in a partial last time tile, with a row pitch padded by 0,
    by nearly nothing and by nearly 16 bytes.  The workspace passed in is
    larger than required and full of 0xFF bytes (NaN as float32, 255 as
    bytes): the result is that of an exact-size workspace and the reference,
    so nothing past the rows' written pitch reaches an output."""
    from riptide_amd import engine
    esize = ESIZE[kind]
    nchans = 5
    max_delay = (dc.LAST_STAGED[esize] + 40) if direct else 40
    unit = 16 if esize == 1 else 4
    nsamp = (max_delay + NOUT) // unit * unit + rem
    if rem > 1:
        nsamp -= unit
    nout = nsamp - max_delay
    assert nsamp % unit == rem and nout % dc.TIME_TILE and nout > dc.TIME_TILE
    delays = np.stack([np.arange(nchans), (np.arange(nchans) * 7) % 19 + 1,
                       np.full(nchans, max_delay)]).astype(np.int64)
    assert delays.min() == 0 and delays.max() == max_delay
    paths = dc.tile_paths(delays, max_delay, esize)
    assert set(paths.ravel()) == ({"D"} if direct else {"S"})
    x = dc.samples(np.random.RandomState(rem), nsamp, nchans, kind)
    need = engine.dedisperse_workspace_bytes(kind, nsamp, nchans)
    assert need == -(-nsamp * esize // 16) * 16 * nchans
    poisoned = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    out = run(torch, x, delays, max_delay, workspace=poisoned)
    exact = run(torch, x, delays, max_delay, workspace=torch.zeros(need, dtype=torch.uint8, device="cuda"))
    assert np.all(poisoned[need:].cpu().numpy() == 0xFF)       # nothing written behind the rows either
    dc.assert_same_bits(out, exact, "poisoned oversize workspace against an exact-size one")
    if esize == 4:
        ref = dc.numpy_dedisperse_f32(x, delays, nout)
    else:
        ref = dc.numpy_dedisperse(x, delays, nout)[0].astype(np.float32)
    dc.assert_same_bits(out, ref, "device against numpy")
    assert np.all(np.isfinite(out))


@pytest.mark.parametrize("kind", ["uint8", "float32"])
def test_delay_clamp(torch, kind):
    """include/riptide_amd.h: the device call clamps delay entries to [0,
    max_delay].  A table with -1, -2^31, max_delay + 1 and 2^31 - 1 in real DM
    rows of staged and of direct channels gives the bits of its np.clip, which
    are the host specification's on the clipped table."""
    from riptide_amd.dedispersion import dedisperse_host
    esize = ESIZE[kind]
    wild, max_delay = dc.clamp_table(esize)
    clipped = np.clip(wild, 0, max_delay)
    bad = (wild != clipped).any(axis=0)
    paths = dc.tile_paths(wild, max_delay, esize)
    assert {"S", "D"} <= set(paths[0, bad]) and bad.all()
    x = dc.samples(np.random.RandomState(3), max_delay + NOUT, wild.shape[1], kind)
    out = run(torch, x, wild, max_delay)
    dc.assert_same_bits(out, run(torch, x, clipped, max_delay), "wild table against its clip")
    dc.assert_same_bits(out, dedisperse_host(x, clipped, max_delay), "against the host specification")
    if esize == 4:
        dc.assert_same_bits(out, dc.numpy_dedisperse_f32(x, clipped, NOUT), "against numpy")
    else:
        dc.assert_same_bits(out, dc.numpy_dedisperse(x, clipped, NOUT)[0].astype(np.float32), "against numpy")


@pytest.mark.parametrize("kind", ["float32", "u16", "uint8-zero_dm", "int8-zero_dm", "u4-zero_dm"])
def test_float_rows_bit_identity(torch, kind):
    """float32 results are summed in channel order: the device sums of float
    rows -- float32 and 16-bit data, and every type under the zero-DM filter
    -- have the bits of one float32 accumulator taking the channels in
    ascending order, staged and direct channels alike, plain and through the
    band table, with and without the mask."""
    kind, _, zero_dm = kind.partition("-")
    for r, ndm in ((1, 17), (2, 5)):
        delays, mask, max_delay = dc.threshold_table(4, r, ndm)
        paths = dc.tile_paths(delays, max_delay, 4, mask)
        assert {"S", "D", "M"} <= set(paths[0, :16]) and {"S", "D"} <= set(paths[0, 16:])
        for m in (mask, None):
            check(torch, kind, delays, max_delay, m, zero_dm=bool(zero_dm), seed=ndm)
            out = check(torch, kind, delays, max_delay, m, bands=BAND_TABLE, zero_dm=bool(zero_dm), seed=ndm)
            assert not out[:, 4].any()


def test_nan_and_inf_reach_their_outputs_alone(torch):
    """One NaN sample in a direct channel and one +inf sample in a staged one:
    exactly the outputs (d, t - delay[d, c]) that read them are NaN or +inf,
    every other output keeps the bits of the reference."""
    delays, mask, max_delay = dc.threshold_table(4, 3, 16)
    paths = dc.tile_paths(delays, max_delay, 4, mask)
    c_nan, c_inf, t_nan, t_inf = 4, 5, 280, 290     # behind every delay of their channels (at most 275)
    assert paths[0, c_nan] == "D" and paths[0, c_inf] == "S"
    x = dc.samples(np.random.RandomState(7), max_delay + NOUT, delays.shape[1], np.float32)
    x[t_nan, c_nan] = np.nan
    x[t_inf, c_inf] = np.inf
    out = run(torch, x, delays, max_delay, mask)
    want_nan = np.zeros(out.shape, dtype=bool)
    want_inf = np.zeros(out.shape, dtype=bool)
    for d in range(delays.shape[0]):
        for want, t, c in ((want_nan, t_nan, c_nan), (want_inf, t_inf, c_inf)):
            if 0 <= t - delays[d, c] < NOUT:
                want[d, t - delays[d, c]] = True
    want_inf &= ~want_nan
    assert want_nan.sum() >= 8 and want_inf.sum() >= 8
    assert np.array_equal(np.isnan(out), want_nan)
    assert np.array_equal(out == np.inf, want_inf) and not np.any(out == -np.inf)
    ref = dc.numpy_dedisperse_f32(x, delays, NOUT, mask)
    keep = ~want_nan
    assert np.array_equal(dc.bits(out)[keep], dc.bits(ref)[keep])
