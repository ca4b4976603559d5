"""Shared by the injection tests (test_inject_host.py, test_gpu_inject.py): a
plain numpy restatement of the specification (include/riptide_amd.h, "signal
injection") -- int64 / uint64 arithmetic that wraps, np.rint, float32
products and sums in signal order -- independent of the C code and the
yardstick for both; the signal tables of the bit-equality cases; and the small
filterbank files of the file-level tests."""
import numpy as np

import dedisp_common as dc

GOLDEN = 0x9E3779B97F4A7C15
SPAN = 4096
EDGE = (1.0 - 2.0 ** -20) / SPAN            # |f| * span just under 1
SMALL = 1e-9
DTYPES = ["uint8", "int8", "float32"]
NCHANS = [1, 3, 63, 64, 65, 130]


def numpy_inject(x, T, t_origin=0, seed=0):
    """The specification on a numpy block: a new array."""
    x = np.array(x, copy=True)
    g, n = x.shape
    t = (np.int64(t_origin) + np.arange(g, dtype=np.int64))[:, None]
    acc = np.zeros((g, n), dtype=np.float32)
    with np.errstate(over="ignore"):
        for sp in T.specs:
            d = T.delay[int(sp["delay_off"]):int(sp["delay_off"]) + n].astype(np.int64)[None, :]
            a = T.amp[int(sp["amp_off"]):int(sp["amp_off"]) + n][None, :]
            u = t - d
            ue = u
            if float(sp["factor"]) != 0.0:
                q = u * (np.int64(sp["span"]) - u)
                ue = u + np.rint(np.float64(sp["factor"]) * q.astype(np.float64)).astype(np.int64)
            tp = T.tmpl[int(sp["tmpl_off"]):]
            if int(sp["kind"]) == 0:
                ph = np.uint64(sp["phase0"]) + ue.astype(np.uint64) * np.uint64(sp["step"])
                v = a * tp[(ph >> np.uint64(64 - int(sp["log2bins"]))).astype(np.int64)]
            else:
                i = ue - np.int64(sp["t0"])
                L = int(sp["length"])
                v = np.where((i >= 0) & (i < L), a * tp[np.clip(i, 0, L - 1)], np.float32(0.0))
            assert v.dtype == np.float32
            acc = acc + v
        if x.dtype == np.float32:
            return x + acc
        z = (t.astype(np.uint64) * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :]
             + np.uint64(int(seed) * GOLDEN % (1 << 64)))
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    r = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    inc = np.floor(np.fmin(np.fmax(acc + r, np.float32(-65536.0)), np.float32(65536.0))).astype(np.int32)
    info = np.iinfo(x.dtype)
    return np.clip(x.astype(np.int32) + inc, info.min, info.max).astype(x.dtype)


def raw_tables(K, nchans, g, t_origin, log2bins, seed=0, scale=3.0):
    """(specs, tmpl, amp, delay) of K signals, kinds alternating from periodic:
    amplitudes of both signs, delays from below zero to several block lengths,
    a phase that wraps 2^64 within the block, pulse windows (signals 1, 3, 5,
    7) partly before row 0, partly past the last row, wholly outside and
    inside, and the factors 0, +EDGE, -EDGE, +SMALL, -SMALL in turn (signals 0
    to 4): K = 9 has every placement and every factor, which covers_edges
    asserts on the tables a test uses."""
    from riptide_amd.engine import INJECT_SPEC_DTYPE
    rng = np.random.RandomState(1000 * K + 10 * nchans + log2bins + seed)
    specs = np.zeros(K, dtype=INJECT_SPEC_DTYPE)
    tmpl, amp, delay = [], [], []
    factors = [0.0, EDGE, -EDGE, SMALL, -SMALL]
    for k in range(K):
        sp = specs[k]
        sp["kind"] = k & 1
        sp["tmpl_off"] = sum(t.size for t in tmpl)
        sp["amp_off"] = sp["delay_off"] = k * nchans
        if k & 1:
            where = (k // 2) % 4
            # a window of one entry (the shortest) where it lies inside; two or more where it straddles an end
            L = 1 if where == 3 else int(rng.randint(2, 40))
            sp["length"] = L
            tmpl.append(rng.uniform(-0.5, 1.5, size=L).astype(np.float32))
            sp["t0"] = t_origin + [-(L // 2), g - (L + 1) // 2, g + 100, g // 3][where]
        else:
            sp["log2bins"] = log2bins
            tmpl.append(rng.uniform(-0.5, 1.5, size=1 << log2bins).astype(np.float32))
            sp["step"] = int(rng.randint(1, 1 << 62)) * 4 + 1
            # just below 2^64 at u = t_origin + g // 2: a channel whose delay is within half a block of zero wraps
            sp["phase0"] = ((1 << 64) - 1 - int(rng.randint(0, 1 << 16)) - (t_origin + g // 2) * int(sp["step"])) % (1 << 64)
        amp.append((rng.uniform(-1.0, 1.0, size=nchans) * scale).astype(np.float32))
        delay.append(rng.randint(-g, 3 * g + 7, size=nchans).astype(np.int32))
        sp["factor"] = factors[k % len(factors)]
        sp["span"] = SPAN
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return specs, cat(tmpl, np.float32), cat(amp, np.float32), cat(delay, np.int32)


def covers_edges(raw, g, t_origin):
    """Asserts on a raw_tables result of K >= 9 and g >= 40 what it is meant to
    hit: both kinds, all five factors, amplitudes of both signs, the four
    window placements, and a phase that passes 2^64 inside the block."""
    # (the phase's quotient by 2^64 differs between the block's first and last row)
    specs, _, amp, _ = raw
    assert set(specs["kind"]) == {0, 1} and set(specs["factor"]) == {0.0, EDGE, -EDGE, SMALL, -SMALL}
    assert abs(EDGE) * SPAN < 1.0 and (amp > 0).any() and (amp < 0).any()
    pulses = specs[specs["kind"] == 1]
    t0, L = pulses["t0"] - t_origin, pulses["length"].astype(np.int64)
    assert ((t0 < 0) & (t0 + L > 0)).any() and ((t0 < g) & (t0 + L > g)).any() and (t0 >= g).any()
    assert ((t0 >= 0) & (t0 + L <= g)).any() and L.min() == 1
    # signal 0's phase passes 2^64 inside the block in some channel (one with a delay near zero), once there are
    # channels enough for such a delay to be drawn
    nchans = amp.size // specs.size
    if nchans >= 63:
        sp, d = specs[0], raw[3][:nchans]
        assert any(len({(int(sp["phase0"]) + (t - int(dc_)) * int(sp["step"])) >> 64
                        for t in (t_origin, t_origin + g - 1)}) > 1 for dc_ in d if -(g // 2) <= dc_ < g // 2)


def tables(K, nchans, g, t_origin, log2bins, seed=0, scale=3.0):
    from riptide_amd.injection import InjectionTables
    return InjectionTables(*raw_tables(K, nchans, g, t_origin, log2bins, seed, scale), nchans)


def block(g, nchans, dtype, seed=0):
    """Samples with the ends of the range among them (saturation both ways)."""
    rng = np.random.RandomState(seed + g + nchans)
    if np.dtype(dtype) == np.float32:
        return rng.normal(0.0, 10.0, size=(g, nchans)).astype(np.float32)
    info = np.iinfo(dtype)
    x = rng.randint(info.min, info.max + 1, size=(g, nchans))
    ends = rng.randint(0, 6, size=(g, nchans))
    x = np.where(ends == 0, info.min, np.where(ends == 1, info.max, np.where(ends == 2, info.min + 1,
                                                                             np.where(ends == 3, info.max - 1, x))))
    return x.astype(dtype)


def saturation_case(dtype):
    """(x, tables): every sample at an end of the range or next to it, one
    constant signal per sign and size: +-0.7 and +-300 (beyond the range)."""
    from riptide_amd.engine import INJECT_SPEC_DTYPE
    from riptide_amd.injection import InjectionTables
    info = np.iinfo(dtype)
    ends = np.array([info.min, info.min + 1, info.max - 1, info.max])
    nchans, g = 8, 64
    x = np.tile(ends, (g, 2)).astype(dtype)
    out = []
    for a in (0.7, -0.7, 300.0, -300.0):
        specs = np.zeros(1, dtype=INJECT_SPEC_DTYPE)
        specs[0]["log2bins"], specs[0]["step"], specs[0]["span"] = 1, 12345, SPAN
        out.append(InjectionTables(specs, np.ones(2, dtype=np.float32), np.full(nchans, a, dtype=np.float32),
                                   np.zeros(nchans, dtype=np.int32), nchans))
    return x, out


def header(x, **extra):
    nchans = x.shape[1]
    h = {"source_name": "fake", "src_raj": 0.0, "src_dej": 0.0, "tstart": 60000.0, "tsamp": dc.TSAMP,
         "nbits": 8 * x.dtype.itemsize, "fch1": 400.0, "foff": -32.0 / nchans, "nchans": nchans, "nifs": 1}
    if x.dtype == np.int8:
        h["signed"] = True
    h.update(extra)
    return h


def write_filterbank(path, x, **extra):
    from riptide_amd.reading import write_sigproc
    write_sigproc(str(path), x, header(x, **extra))
    return str(path)
