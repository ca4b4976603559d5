"""Shared by the block-mask tests: the numpy restatement of the replacement a
block mask stands for (rt_block_mask in include/riptide_amd.h),

  x'[t, c] = fill[c]  if cells[(t_origin + t) // block_len, c]  else  x[t, c],

of the block statistics in the summation order the header states, and the
masks and sample sets the host and the GPU tests both use."""
import numpy as np

from riptide_amd import reading

STATS_CHUNK = 2048

# sample families: (name, numpy dtype of the values, nbits or None)
FAMILIES = {"uint8": (np.uint8, None), "int8": (np.int8, None), "float32": (np.float32, None),
            "u1": (np.uint8, 1), "u2": (np.uint8, 2), "u4": (np.uint8, 4), "u16": (np.uint16, 16)}
DTYPE_CODES = {"uint8": 0, "int8": 1, "float32": 2, "u1": 0x101, "u2": 0x102, "u4": 0x104, "u16": 0x110}


def whole_bytes(family, nchans):
    """nchans rounded up to rows of whole bytes for the 1/2/4-bit families
    (1 -> 8, 4, 2 and 65 -> 72, 68, 66), nchans itself for every other."""
    nbits = FAMILIES[family][1]
    if nbits in (1, 2, 4):
        per = 8 // nbits
        return -(-nchans // per) * per
    return nchans


def values(rng, family, nsamp, nchans):
    """Random sample values [nsamp, nchans] of a family (unpacked)."""
    dtype, nbits = FAMILIES[family]
    if family == "float32":
        return rng.normal(size=(nsamp, nchans)).astype(np.float32)
    if nbits is not None:
        return rng.randint(0, 1 << nbits, size=(nsamp, nchans)).astype(dtype)
    info = np.iinfo(dtype)
    return rng.randint(info.min, info.max + 1, size=(nsamp, nchans)).astype(dtype)


def fill_of(rng, family, nchans):
    """A fill in the family's own type; packed 1/2/4-bit fills carry high bits
    that must be ignored."""
    dtype, nbits = FAMILIES[family]
    if family == "float32":
        return rng.normal(size=nchans).astype(np.float32)
    if nbits == 16:
        return rng.randint(0, 1 << 16, size=nchans).astype(np.uint16)
    if nbits is not None:
        return rng.randint(0, 256, size=nchans).astype(np.uint8)
    info = np.iinfo(dtype)
    return rng.randint(info.min, info.max + 1, size=nchans).astype(dtype)


def as_block(x, family):
    """The array an entry point takes: packed rows for the packed families."""
    nbits = FAMILIES[family][1]
    return x if nbits is None else reading.pack_samples(x, nbits)


def as_values(block, family, nchans):
    nbits = FAMILIES[family][1]
    return block if nbits is None else reading.unpack_samples(block, nbits, nchans)


def numpy_replace(x, cells, block_len, fill, t_origin=0, nbits=None):
    """x' of unpacked values x [nsamp, nchans]."""
    fill = np.asarray(fill)
    if nbits is not None and nbits < 16:
        fill = fill & ((1 << nbits) - 1)
    blk = (t_origin + np.arange(x.shape[0])) // block_len
    flags = np.asarray(cells, dtype=bool)[blk]          # [nsamp, nchans]
    return np.where(flags, fill.astype(x.dtype)[None, :], x)


def nblocks_for(nsamp, block_len, t_origin):
    return -(-(t_origin + nsamp) // block_len)


def mask_kinds(rng, nblocks, nchans):
    """none, all, one cell, one whole block, one whole channel, random 30 %."""
    none = np.zeros((nblocks, nchans), dtype=bool)
    one = none.copy()
    one[nblocks // 2, nchans // 2] = True
    block = none.copy()
    block[nblocks - 1] = True
    chan = none.copy()
    chan[:, nchans // 3] = True
    return {"none": none, "all": ~none, "cell": one, "block": block, "channel": chan,
            "random": rng.rand(nblocks, nchans) < 0.3}


def numpy_block_stats(x, block_len):
    """float64 [nblk, 2, nchans] of values x [nsamp, nchans].  Integer values:
    exact int64 sums.  float32: the header's order -- chunks of 2048 rows from
    the block's first row, row j of a chunk added to partial sum j mod 4 from
    0.0, ((p0 + p1) + p2) + p3, the chunks added in order from 0.0."""
    nsamp, nchans = x.shape
    nblk = -(-nsamp // block_len)
    out = np.zeros((nblk, 2, nchans), dtype=np.float64)
    for b in range(nblk):
        rows = x[b * block_len:min((b + 1) * block_len, nsamp)]
        if x.dtype.kind in "iu":
            v = rows.astype(np.int64)
            out[b, 0], out[b, 1] = v.sum(axis=0), (v * v).sum(axis=0)
            continue
        v = rows.astype(np.float64)
        s, q = np.zeros(nchans), np.zeros(nchans)
        for t0 in range(0, v.shape[0], STATS_CHUNK):
            chunk = v[t0:t0 + STATS_CHUNK]
            ps, pq = np.zeros((4, nchans)), np.zeros((4, nchans))
            for j in range(chunk.shape[0]):
                ps[j & 3] += chunk[j]
                pq[j & 3] += chunk[j] * chunk[j]
            s += ((ps[0] + ps[1]) + ps[2]) + ps[3]
            q += ((pq[0] + pq[1]) + pq[2]) + pq[3]
        out[b, 0], out[b, 1] = s, q
    return out
