"""Shared by the dedispersion tests: the numpy restatement they compare
against, the band they use and the float32 bound."""
import numpy as np

KDM = 1.0 / 2.41e-4
TSAMP = 1e-3


def band(nchans, ascending=False):
    """nchans channel centres of a 368-400 MHz band; DM 50 spans about 230
    samples of 1 ms across it."""
    step = 32.0 / nchans
    return 368.0 + step * np.arange(nchans) if ascending else 400.0 - step * np.arange(nchans)


def numpy_delays(freqs, dms, tsamp, kdm=KDM):
    freqs = np.asarray(freqs, dtype=np.float64)
    f_ref = freqs.max()
    out = np.zeros((len(dms), freqs.size), dtype=np.int64)
    for d, dm in enumerate(dms):
        for c, f in enumerate(freqs):
            a = 1.0 / (f * f) - 1.0 / (f_ref * f_ref)
            out[d, c] = int(np.floor(kdm * float(dm) * a / tsamp + 0.5))
    return out


def numpy_dedisperse(x, delays, nout, mask=None):
    """(float64 sums [ndm, nout], float64 sums of |x|): exact for 8-bit data."""
    ndm, nchans = delays.shape
    acc = np.zeros((ndm, nout), dtype=np.float64)
    mag = np.zeros((ndm, nout), dtype=np.float64)
    for d in range(ndm):
        for c in range(nchans):
            if mask is not None and mask[c]:
                continue
            col = x[delays[d, c]:delays[d, c] + nout, c].astype(np.float64)
            acc[d] += col
            mag[d] += np.abs(col)
    return acc, mag


def numpy_dedisperse_f32(x, delays, nout, mask=None, bands=None, mean=None):
    """The float32 sums as include/riptide_amd.h defines them, restated: per
    output a float32 accumulator that starts at +0.0 and takes one float32
    addition per unmasked channel, in ascending channel order.  x [nsamp,
    nchans] holds values float32 represents exactly (float32, or 8- and 16-bit
    integers).  bands (uint32 [nbands, 2], channel ranges [lo, hi)): the result
    is [ndm, nbands, nout] instead of [ndm, nout], every band summed from its
    first channel.  mean (float32 [nsamp], the zero-DM mean series): y =
    float32(x[t, c]) - mean[t], one float32 subtraction, is what is added."""
    ndm, nchans = delays.shape
    x32 = np.asarray(x).astype(np.float32)
    if mean is not None:
        mean = np.asarray(mean)
        assert mean.dtype == np.float32 and mean.shape == (x32.shape[0],)
    table = [(0, nchans)] if bands is None else [(int(lo), int(hi)) for lo, hi in bands]
    out = np.zeros((ndm, len(table), nout), dtype=np.float32)
    for d in range(ndm):
        for b, (lo, hi) in enumerate(table):
            acc = np.zeros(nout, dtype=np.float32)
            for c in range(lo, hi):
                if mask is not None and mask[c]:
                    continue
                k = int(delays[d, c])
                col = x32[k:k + nout, c]
                if mean is not None:
                    col = col - mean[k:k + nout]
                acc = acc + col
                assert acc.dtype == np.float32
            out[d, b] = acc
    return out[:, 0] if bands is None else out


def numpy_zero_dm_mean(x, mask=None):
    """m[t] = float32(S[t] / Nu) of integer samples x [nsamp, nchans]: S the
    exact sum of row t over the unmasked channels, Nu their number, divided in
    float64 and rounded once (RT_DEDISP_ZERO_DM, include/riptide_amd.h)."""
    x = np.asarray(x)
    assert x.dtype.kind in "iu"
    keep = np.ones(x.shape[1], dtype=bool) if mask is None else ~np.asarray(mask, dtype=bool)
    nu = int(keep.sum())
    if not nu:
        return np.zeros(x.shape[0], dtype=np.float32)
    s = x[:, keep].astype(np.int64).sum(axis=1)
    return (s.astype(np.float64) / np.float64(nu)).astype(np.float32)


def bits(a):
    """float32 array -> its bits, for comparisons that tell -0.0 from +0.0."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def assert_same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == ref.shape, \
        (what, got.dtype, got.shape, ref.dtype, ref.shape)
    differ = bits(got) != bits(ref)
    if differ.any():
        first = tuple(int(i) for i in np.argwhere(differ)[0])
        raise AssertionError(f"{what}: {int(differ.sum())} of {got.size} sums differ in their bits, the first at "
                             f"{first}: {got[first]!r} against {ref[first]!r}")


def assert_dedispersed(out, x, delays, nout, mask=None):
    """Bit for bit for 8-bit data.  For float data |out - ref64| <= nchans *
    2^-24 * sum |x| (recursive summation in float32), and the bits of
    numpy_dedisperse_f32: the additions themselves, in channel order."""
    ref, mag = numpy_dedisperse(x, delays, nout, mask)
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == ref.shape, (out.dtype, out.shape, ref.shape)
    if x.dtype == np.float32:
        assert np.all(np.isfinite(out))
        err = np.abs(out.astype(np.float64) - ref)
        bound = delays.shape[1] * 2.0 ** -24 * mag
        assert np.all(err <= bound), f"max excess {float((err - bound).max()):.3e}"
        assert_same_bits(out, numpy_dedisperse_f32(x, delays, nout, mask), "float32 sums in channel order")
    else:
        assert np.array_equal(out, ref.astype(np.float32)), \
            f"{int((out != ref.astype(np.float32)).sum())} of {out.size} sums differ"


def samples(rng, nsamp, nchans, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return rng.normal(size=(nsamp, nchans)).astype(np.float32)
    info = np.iinfo(dtype)
    return rng.randint(info.min, info.max + 1, size=(nsamp, nchans)).astype(dtype)


def kind_samples(rng, nsamp, nchans, kind):
    """(what the entry points take, its values [nsamp, nchans], nbits or None)
    of seeded samples of a sample type by name: 'uint8', 'int8', 'float32', or
    packed 'u1', 'u2', 'u4', 'u16' (reading.pack_samples rows)."""
    if kind in ("u1", "u2", "u4", "u16"):
        from riptide_amd.reading import pack_samples
        nbits = int(kind[1:])
        vals = rng.randint(0, 1 << nbits, size=(nsamp, nchans)).astype(np.uint16 if nbits == 16 else np.uint8)
        return pack_samples(vals, nbits), vals, nbits
    x = samples(rng, nsamp, nchans, kind)
    return x, x, None


# ---- hand-made delay tables that put dedisp_sum_kernel on a named path
# The sum kernel works on tiles of DM_TILE DMs x TIME_TILE outputs, CHAN_STEP
# channels at a time.  Per channel it takes lo and hi, the smallest and largest
# clamped delay of the tile's DMs (a partial tile repeats its last DM), and
# either stages the channel's span in LDS or reads the row directly:
# engine.dedisperse_span_plan(esize, lo, hi) is that rule.
DM_TILE, TIME_TILE, CHAN_STEP = 16, 256, 16
SPAN_DWORDS = {1: 264, 4: 520}          # staged dwords of a channel, by element size
# the largest staged hi - (lo & ~(4 / esize - 1)): 264 * 4 - 256 and 520 - 256
LAST_STAGED = {1: 800, 4: 264}

# Classes of the threshold table's channels: S at the last staged spread
# (ndw == SPAN_DWORDS), D one sample beyond it, M masked.  The first
# 16-channel step holds all three, the partial step of four both S and D; M
# next to D at 11, 12 makes [11, 13) a band whose unmasked channels are all D.
THRESHOLD_CLASSES = "SDMSDSMDSDSDMSDS" + "SDDS"


def threshold_table(esize, r, ndm, nchans=20):
    """(delays int64 [ndm, nchans], mask bool [nchans], max_delay): channel c
    has lo_c = r + 4 * (c % 3), so lo_c % 4 == r, and in the first DM tile the
    first DM at lo_c, the last DM of that tile (DM 15, or DM ndm - 1 of fewer)
    at hi_c, the rest spread in between.  hi_c - (lo_c & ~3) is LAST_STAGED for
    a class S channel (hi_c - lo_c for float rows) and one more for D and M.
    DMs from 16 on sit at lo_c + 7 + c: a tile of its own, staged."""
    assert esize in (1, 4) and 0 <= r < 4 and ndm >= 2
    delays = np.zeros((ndm, nchans), dtype=np.int64)
    mask = np.zeros(nchans, dtype=bool)
    n0 = min(ndm, DM_TILE)
    for c in range(nchans):
        cls = THRESHOLD_CLASSES[c % len(THRESHOLD_CLASSES)]
        lo = r + 4 * (c % 3)
        base = lo & ~3 if esize == 1 else lo
        hi = base + LAST_STAGED[esize] + (0 if cls == "S" else 1)
        for k in range(n0):
            delays[k, c] = lo + (k * (hi - lo)) // (n0 - 1)
        delays[n0:, c] = lo + 7 + c
        mask[c] = cls == "M"
    return delays, mask, int(delays.max())


def residue_table(nchans=20, ndm=19):
    """(delays int64 [ndm, nchans], max_delay): delay[d, c] = lo_c + d for the
    16 DMs of the first tile, lo_c = 7 * c % 29 (every lo_c % 4, not monotone
    in c), so every pair (lo_c % 4, (delay - lo_c) % 4) -- the rounding of the
    staged base and the byte residue of the aligned read -- occurs; later DMs
    at lo_c + 5 * d % 16.  Every spread is at most 15 samples: all staged."""
    lo = (7 * np.arange(nchans)) % 29
    d = np.arange(ndm)
    step = np.where(d < DM_TILE, d, (5 * d) % 16)
    delays = (lo[None, :] + step[:, None]).astype(np.int64)
    return delays, int(delays.max())


def clamp_table(esize):
    """(wild int64 [16, 20], max_delay): a table with entries outside [0,
    max_delay] in real DM rows -- -1, -2^31, max_delay + 1, 2^31 - 1 -- whose
    np.clip(., 0, max_delay) has channels on both paths.  Channel c % 3 == 0:
    delays from 0 to LAST_STAGED (staged), the negative entries in rows 3 and
    9 clip to its lo.  c % 3 == 1: from max_delay - LAST_STAGED to max_delay
    (staged), the entries above max_delay in rows 4 and 11 clip to its hi.
    c % 3 == 2: from 0 to max_delay (direct), all four."""
    s = LAST_STAGED[esize]
    max_delay = s + 8
    wild = np.zeros((DM_TILE, 20), dtype=np.int64)
    for c in range(20):
        lo, hi = ((0, s), (max_delay - s, max_delay), (0, max_delay))[c % 3]
        wild[:, c] = lo + (np.arange(DM_TILE) * (hi - lo)) // (DM_TILE - 1)
        if c % 3 != 1:
            wild[3, c], wild[9, c] = -1, -2 ** 31
        if c % 3 != 0:
            wild[4, c], wild[11, c] = max_delay + 1, 2 ** 31 - 1
    return wild, max_delay


def tile_paths(delays, max_delay, esize, mask=None):
    """[number of DM tiles, nchans] of 'S' (staged), 'D' (direct) and 'M'
    (masked): the path of every (DM tile, channel) of a call with this table,
    named by engine.dedisperse_span_plan from the clamped delays of the tile's
    DMs (the rows a partial tile repeats change neither lo nor hi)."""
    from riptide_amd import engine
    delays = np.clip(np.asarray(delays, dtype=np.int64), 0, max_delay)
    ndm, nchans = delays.shape
    ntiles = -(-ndm // DM_TILE)
    paths = np.empty((ntiles, nchans), dtype="U1")
    for k in range(ntiles):
        rows = delays[k * DM_TILE:(k + 1) * DM_TILE]
        for c in range(nchans):
            if mask is not None and mask[c]:
                paths[k, c] = "M"
            else:
                paths[k, c] = "S" if engine.dedisperse_span_plan(esize, rows[:, c].min(), rows[:, c].max())[1] else "D"
    return paths


def path_tables():
    """Every hand-made table of the path tests, by name:
    (delays, mask or None, max_delay, esize, claims), claims a set of
    'mixed' (one 16-channel step of one DM tile holds a staged, a direct and a
    masked channel), 'residues' (every (lo % 4, (delay - lo) % 4) pair occurs,
    all channels staged) and 'clamp' (entries outside [0, max_delay])."""
    tables = {}
    for esize in (1, 4):
        for r in range(4):
            for ndm in (16, 17, 5):
                d, m, md = threshold_table(esize, r, ndm)
                tables[f"threshold-e{esize}-r{r}-ndm{ndm}"] = (d, m, md, esize, {"mixed"})
        d, m, md = threshold_table(esize, 1, 16, nchans=32)
        tables[f"threshold-e{esize}-32ch"] = (d, None, md, esize, set())
        wild, md = clamp_table(esize)
        tables[f"clamp-e{esize}"] = (wild, None, md, esize, {"clamp"})
    for nchans in (20, 32):
        d, md = residue_table(nchans)
        tables[f"residues-{nchans}ch"] = (d, None, md, 1, {"residues"})
    return tables
