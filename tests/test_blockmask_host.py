"""CPU-only tests of the block mask: rt_block_replace_host and
rt_block_stats_host against the numpy restatements of blockmask_common, the
host rule rfi.block_mask on seeded data, BlockMask's fill, typed fill and
save/load, every ValueError, and the sanitizer program.  No call reaches the
GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import blockmask_common as bc
from conftest import REPO

NSAMP = 600


@pytest.fixture(scope="module")
def lib():
    from riptide_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("family", list(bc.FAMILIES))
def test_replace_host(family):
    """rt_block_replace_host equals the numpy restatement bit for bit: every
    sample family (packed input compared after reading.unpack_samples),
    block_len in {1, 7, 256, >= nsamp}, t_origin in {0, 5, block_len - 1},
    masks none / all / one cell / one block / one channel / random 30 %."""
    from riptide_amd import rfi
    nbits = bc.FAMILIES[family][1]
    nchans = 24
    rng = np.random.RandomState(17)
    x = bc.values(rng, family, NSAMP, nchans)
    block = bc.as_block(x, family)
    fill = bc.fill_of(rng, family, nchans)
    for block_len in (1, 7, 256, NSAMP + 50):
        for t_origin in sorted({0, 5, block_len - 1}):
            nblocks = bc.nblocks_for(NSAMP, block_len, t_origin)
            for kind, cells in bc.mask_kinds(rng, nblocks, nchans).items():
                got = rfi.apply_block_mask_host(block, cells, block_len, fill, t_origin=t_origin, nbits=nbits)
                assert got.dtype == block.dtype and got.shape == block.shape
                ref = bc.numpy_replace(x, cells, block_len, fill, t_origin, nbits)
                assert np.array_equal(bc.as_values(got, family, nchans), ref), (block_len, t_origin, kind)
                if kind == "none":
                    assert np.array_equal(got, block)
    # more blocks than the rows need are fine; the input is left alone
    before = block.copy()
    rfi.apply_block_mask_host(block, np.ones((NSAMP, nchans), dtype=bool), 7, fill, nbits=nbits)
    assert np.array_equal(block, before)


def _stats_host(lib, block, family, nsamp, nchans, block_len):
    from riptide_amd import _lib
    nblk = -(-nsamp // block_len)
    out = np.full((nblk, 2, nchans), -7.0, dtype=np.float64)     # written, not accumulated
    assert lib.rt_block_stats_host(_lib.ptr(block), bc.DTYPE_CODES[family], nsamp, nchans, block_len,
                                   _lib.ptr(out)) == _lib.RT_OK, lib.rt_last_error()
    return out


@pytest.mark.parametrize("nchans", [1, 65])
@pytest.mark.parametrize("family", list(bc.FAMILIES))
def test_block_stats_host(lib, family, nchans):
    """rt_block_stats_host against numpy for every sample type: exact int64
    sums for the integer types, the stated summation order restated in numpy
    bit for bit for float32; about 6000 samples, so every block_len leaves a
    partial block."""
    nsamp = 6000
    nchans = bc.whole_bytes(family, nchans)
    x = bc.values(np.random.RandomState(nchans), family, nsamp, nchans)
    block = bc.as_block(x, family)
    for block_len in (1, 5, 2048, 2049, 5000):
        got = _stats_host(lib, block, family, nsamp, nchans, block_len)
        assert np.array_equal(got, bc.numpy_block_stats(x, block_len)), block_len
    one = _stats_host(lib, block, family, nsamp, nchans, 10 * nsamp)
    assert one.shape[0] == 1 and np.array_equal(one, bc.numpy_block_stats(x, nsamp))


def _seeded(seed, tail=0):
    """uint8 rint(normal(100, 10)), 64 blocks x 32 channels x 256 samples (+ a
    partial tail): + 15 in blocks 10-12 of channels 3-5, block 20 of channel 9
    with its deviation from 100 doubled."""
    nblocks, nchans, blen = 64, 32, 256
    d = np.random.RandomState(seed).normal(100.0, 10.0, size=(nblocks * blen + tail, nchans))
    d[10 * blen:13 * blen, 3:6] += 15.0
    d[20 * blen:21 * blen, 9] = 100.0 + 2.0 * (d[20 * blen:21 * blen, 9] - 100.0)
    injected = np.zeros((nblocks + (tail > 0), nchans), dtype=bool)
    injected[10:13, 3:6] = True
    injected[20, 9] = True
    return np.rint(d).astype(np.uint8), injected, blen


def _stats_of(lib, x, block_len):
    from riptide_amd import rfi
    s = _stats_host(lib, x, "uint8", x.shape[0], x.shape[1], block_len)
    return rfi.BlockStats(s[:, 0], s[:, 1], block_len, x.shape[0])


@pytest.mark.parametrize("tail", [0, 100])
@pytest.mark.parametrize("seed", range(5))
def test_block_mask_seeded(lib, seed, tail):
    """Every injected cell is flagged and at most 1 % of the clean cells,
    with and without a 100-sample partial tail."""
    from riptide_amd import rfi
    x, injected, blen = _seeded(seed, tail)
    stats = _stats_of(lib, x, blen)
    assert stats.count[-1] == (tail or blen) and stats.nsamp == x.shape[0]
    bm = rfi.block_mask(stats)
    assert bm.cells.shape == injected.shape and bm.block_len == blen
    assert bm.cells[injected].all()
    assert (bm.cells & ~injected).sum() <= 0.01 * (~injected).sum()
    if tail:
        assert np.array_equal(bm.cells[-1], bm.cells[-2])      # the tail takes the flags of the block before
    assert np.all(np.abs(bm.fill - 100.0) < 0.5)
    assert bm.fraction == bm.cells.mean() and not bm.channel_mask().any()


def test_block_mask_promotions(lib):
    """A stuck channel (std 0) is flagged everywhere; a channel flagged in more
    than chan_frac of its blocks and a block flagged in more than block_frac
    of its channels are flagged whole; the fill of a channel with no unflagged
    full block is its mean over the file."""
    from riptide_amd import rfi
    x, _, blen = _seeded(0)
    x = x.copy()
    x[20 * blen:44 * blen, 11] = np.clip(x[20 * blen:44 * blen, 11].astype(int) + 40, 0, 255)   # 24 of 64 blocks
    x[50 * blen:51 * blen, :12] = 250              # 12 of 32 channels of block 50
    x[:, 7] = 42                                   # stuck
    stats = _stats_of(lib, x, blen)
    bm = rfi.block_mask(stats, chan_frac=0.3, block_frac=0.3)
    assert bm.cells[:, 7].all() and bm.channel_mask()[7]
    assert bm.cells[:, 11].all()                   # 24 / 64 > 0.3
    assert bm.cells[50].all()                      # 12 + the two whole channels > 0.3 * 32
    assert bm.fill[7] == 42.0
    assert bm.fill[11] == stats.sum[:, 11].sum() / x.shape[0]
    loose = rfi.block_mask(stats, chan_frac=0.5, block_frac=0.5)
    assert not loose.cells[:, 11].all() and loose.cells[20:44, 11].all()
    assert not loose.cells[50].all() and loose.cells[50, :12].all()
    assert list(np.flatnonzero(loose.channel_mask())) == [7]


def test_fill_types_and_round_trip(tmp_path):
    """typed_fill: rint and a clip to the sample's range for each integer type,
    a float32 cast for float32; save / load round trip."""
    from riptide_amd import rfi
    fill = np.array([-3.5, 0.5, 1.5, 2.5, 99.49, 200.7, 300.0, 70000.0])
    bm = rfi.BlockMask(np.zeros((3, 8), dtype=bool), 100, fill)
    assert bm.typed_fill(np.uint8).tolist() == [0, 0, 2, 2, 99, 201, 255, 255]
    assert bm.typed_fill(np.uint8).dtype == np.uint8
    assert bm.typed_fill(np.int8).tolist() == [-4, 0, 2, 2, 99, 127, 127, 127]
    assert bm.typed_fill(np.int8).dtype == np.int8
    for nbits in (1, 2, 4):
        top = (1 << nbits) - 1
        got = bm.typed_fill(np.uint8, nbits=nbits)
        assert got.dtype == np.uint8 and got.tolist() == [min(max(v, 0), top) for v in (-4, 0, 2, 2, 99, 201, 300, 70000)]
    assert bm.typed_fill(np.uint16, nbits=16).tolist() == [0, 0, 2, 2, 99, 201, 300, 65535]
    assert bm.typed_fill(np.uint16, nbits=16).dtype == np.uint16
    f32 = bm.typed_fill(np.float32)
    assert f32.dtype == np.float32 and np.array_equal(f32, fill.astype(np.float32))
    bm.cells[1, 2] = bm.cells[2, 7] = True
    name = str(tmp_path / "mask.npz")
    bm.save(name)
    back = rfi.BlockMask.load(name)
    assert np.array_equal(back.cells, bm.cells) and back.cells.dtype == bool
    assert back.block_len == 100 and np.array_equal(back.fill, bm.fill)
    assert back.fraction == 2 / 24


def test_value_errors(lib):
    from riptide_amd import _lib, rfi
    x = np.zeros((100, 8), dtype=np.uint8)
    cells = np.zeros((10, 8), dtype=bool)
    fill = np.zeros(8, dtype=np.uint8)
    rfi.apply_block_mask_host(x, cells, 10, fill)
    with pytest.raises(ValueError, match="reach past the mask"):
        rfi.apply_block_mask_host(x, cells, 10, fill, t_origin=1)
    with pytest.raises(ValueError, match="reach past the mask"):
        rfi.apply_block_mask_host(x, cells[:9], 10, fill)
    with pytest.raises(ValueError, match="block_len"):
        rfi.apply_block_mask_host(x, cells, 0, fill)
    with pytest.raises(ValueError, match="cells must be"):
        rfi.apply_block_mask_host(x, cells[:, :7], 10, fill)
    with pytest.raises(ValueError, match="fill must be a uint8"):
        rfi.apply_block_mask_host(x, cells, 10, fill.astype(np.int8))
    with pytest.raises(ValueError, match="fill must be a float32"):
        rfi.apply_block_mask_host(x.astype(np.float32), cells, 10, fill)
    with pytest.raises(ValueError, match="fill must be a uint16"):
        rfi.apply_block_mask_host(np.zeros((100, 16), dtype=np.uint8), cells, 10, fill, nbits=16)
    with pytest.raises(ValueError, match="fill must be"):
        rfi.apply_block_mask_host(x, cells, 10, fill[:7])
    with pytest.raises(ValueError, match="t_origin"):
        rfi.apply_block_mask_host(x, cells, 10, fill, t_origin=-1)
    with pytest.raises(ValueError):
        rfi.BlockMask(cells, 0, np.zeros(8))
    with pytest.raises(ValueError):
        rfi.BlockMask(cells, 10, np.zeros(7))
    with pytest.raises(ValueError, match="t_origin"):
        rfi.apply_block_mask_host(x, cells, 10, fill, t_origin=1 << 64)       # not truncated to 0
    with pytest.raises(ValueError, match="overflows 64 bits"):
        rfi.apply_block_mask_host(x, np.zeros((1, 8), dtype=bool), (1 << 64) - 1, fill, t_origin=(1 << 64) - 50)
    with pytest.raises(ValueError):
        rfi.BlockStats(np.zeros((3, 8)), np.zeros((3, 8)), 10, 100)
    with pytest.raises(ValueError, match="at least 1"):
        rfi.BlockStats(np.zeros((0, 8)), np.zeros((0, 8)), 10, 0)
    with pytest.raises(ValueError, match="at least 1"):
        rfi.BlockStats(np.zeros((1, 8)), np.zeros((1, 8)), 0, 10)
    with pytest.raises(ValueError, match="nbits"):
        rfi.BlockMask(cells, 10, np.zeros(8)).typed_fill(np.uint8, nbits=3)
    # the C entry points themselves
    bm = _lib.BlockMaskStruct(cells.ctypes.data, 10, 10, 0, fill.ctypes.data)
    out = np.zeros_like(x)
    call = lambda: lib.rt_block_replace_host(_lib.ptr(x), 0, 100, 8, ctypes.byref(bm), _lib.ptr(out))
    assert call() == _lib.RT_OK
    assert lib.rt_block_replace_host(_lib.ptr(x), 0, 100, 8, None, _lib.ptr(out)) == _lib.RT_OK
    bm.cells = None
    assert call() == _lib.RT_EINVAL
    bm.cells, bm.fill = cells.ctypes.data, None
    assert call() == _lib.RT_EINVAL
    bm.fill, bm.block_len = fill.ctypes.data, 0
    assert call() == _lib.RT_EINVAL
    bm.block_len = 10
    assert lib.rt_block_replace_host(_lib.ptr(x), 7, 100, 8, ctypes.byref(bm), _lib.ptr(out)) == _lib.RT_EINVAL
    stats = np.zeros((10, 2, 8))
    assert lib.rt_block_stats_host(_lib.ptr(x), 0, 100, 8, 0, _lib.ptr(stats)) == _lib.RT_EINVAL
    assert lib.rt_block_stats_host(_lib.ptr(x), 7, 100, 8, 10, _lib.ptr(stats)) == _lib.RT_EINVAL
    assert lib.rt_block_stats_host(_lib.ptr(x), 0, 100, 0, 10, _lib.ptr(stats)) == _lib.RT_EINVAL


def test_asan_blockmask_check():
    """`make asan` builds build/asan/blockmask_check (g++, AddressSanitizer +
    UBSan, no HIP): rt_block_replace_host and rt_block_stats_host on
    exact-size heap arrays over the edge shapes and every error return."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "blockmask_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("blockmask_check OK")
