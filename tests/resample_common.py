"""Shared by the resampling tests (test_resample_host.py, test_gpu_resample.py):
the sizes and factors of the bit-equality cases, the batch shapes, the special
values, and the accelerated pulse train of the end-to-end test.  The edge
factors are asserted here, on a numpy restatement of the unclamped map, to hit
the edges they are named for."""
import functools

import numpy as np

C = 299792458.0
SIZES = [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4099, 65537]
TIE_N, TIE_F = 1025, 2.0 ** -11


def unclamped(n, f):
    """j - s_j, int64 [n], before the clamp."""
    j = np.arange(n, dtype=np.int64)
    return j - np.rint(np.float64(f) * (j * (n - j)).astype(np.float64)).astype(np.int64)


def edge_factor(n):
    return (1.0 - 2.0 ** -20) / n


def factors(n):
    """The factors of size n's bit-equality case, by name."""
    e = edge_factor(n)
    rnd = float(np.random.RandomState(n).uniform(-1.0, 1.0)) * e
    out = {"zero": 0.0, "tiny+": 1e-300, "tiny-": -1e-300, "edge+": e, "edge-": -e, "random": rnd}
    if n == TIE_N:
        out.update({"tie+": TIE_F, "tie-": -TIE_F})
    return out


# f * q is exactly 0.5 at j = 1 and j = 1024 of N = 1025: half-even gives shift 0, half-away 1
assert TIE_F * float(1 * (TIE_N - 1)) == 0.5 and TIE_F * float(1024 * (TIE_N - 1024)) == 0.5
assert unclamped(TIE_N, TIE_F)[[1, 1024]].tolist() == [1, 1024]
assert unclamped(TIE_N, -TIE_F)[[1, 1024]].tolist() == [1, 1024]
for _n in SIZES:
    assert abs(edge_factor(_n)) * float(_n) < 1.0
    assert not np.any(unclamped(_n, 1e-300) - np.arange(_n)) and not np.any(unclamped(_n, -1e-300) - np.arange(_n))
    assert np.all(np.diff(unclamped(_n, edge_factor(_n))) >= 0) and np.all(np.diff(unclamped(_n, -edge_factor(_n))) >= 0)
    assert unclamped(_n, edge_factor(_n)).min() >= 0
    if _n >= 3:
        # |f| * q at j = N - 1 is just under (N - 1) / N > 1/2: the negative edge factor asks for index N
        # (at N = 2 it is just under 1/2 and rounds to 0; at N = 1, q = 0)
        assert unclamped(_n, -edge_factor(_n))[_n - 1] == _n


def series(B, N, seed, ld=None):
    """float32 [B, N] of seeded noise: a view of a [B, ld] array whose gaps hold NaN."""
    ld = N if ld is None else ld
    wide = np.full((B, ld), np.nan, dtype=np.float32)
    wide[:, :N] = np.random.RandomState(seed).normal(size=(B, N)).astype(np.float32)
    return wide[:, :N]


# (B sources, R rows, N): src repeated, permuted, leaving sources unused; N crosses tiles and is odd
BATCH_SHAPES = [(1, 1, 4099), (1, 7, 4099), (5, 1, 4099), (5, 7, 4099), (1, 300, 1025), (5, 300, 1025)]


def batch_rows(B, R, N, seed=7):
    """(src int32 [R], factor float64 [R]): source 1 of 5 is never used."""
    rng = np.random.RandomState(seed + R)
    pool = np.array([s for s in range(B) if B == 1 or s != 1])
    src = rng.permutation(np.resize(pool, R)).astype(np.int32)
    f = rng.uniform(-1.0, 1.0, size=R) * edge_factor(N)
    f[::5] = 0.0
    return src, f


def special_values(N=1025):
    """float32 [1, N] whose bits must survive: NaNs with payloads, infinities, -0.0, denormals."""
    bits = np.random.RandomState(3).randint(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    bits[:8] = [0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF]
    return bits.view(np.float32)[None, :]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def host_case(n):
    """(x float32 [2, n], names, factors, rt_resample_host's rows [2 * F, n]) of size n, computed once."""
    from riptide_amd import acceleration
    x = series(2, n, 1000 + n)
    fs = factors(n)
    out = acceleration.resample_host(x, list(fs.values()))
    out.setflags(write=False)
    return x, list(fs), np.array(list(fs.values())), out


# ---- the accelerated pulse train
ACC_N, ACC_TSAMP, ACC_PERIOD, ACC_DUCY = 1 << 16, 1e-3, 0.5, 0.05
ACC_TOBS = ACC_N * ACC_TSAMP
# the drift a T^2 / (8 c) at mid-observation is four pulse widths
ACC_A = 4 * ACC_DUCY * ACC_PERIOD * 8.0 * C / ACC_TOBS ** 2
ACC_TRIALS = [-2 * ACC_A, -ACC_A, 0.0, ACC_A, 2 * ACC_A]
ACC_RADIUS = 0.2          # clustering radius, in units of 1 / tobs
ACC_DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}
ACC_RANGES = [{"name": "short",
               "ffa_search": {"period_min": 0.3, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
               "find_peaks": {"smin": 7.0}}]
assert 5e-3 < ACC_A * ACC_TSAMP / (2 * C) * ACC_N < 7e-3


def accel_series(seed=11, amplitude=0.6):
    """Unit noise plus a top-hat pulse train whose phase is
    phi(t) = f (t - a t (t - T) / (2 c)): frequency f = 1 / ACC_PERIOD at mid-observation."""
    t = np.arange(ACC_N, dtype=np.float64) * ACC_TSAMP
    phi = (t - ACC_A * t * (t - ACC_TOBS) / (2 * C)) / ACC_PERIOD
    x = np.random.RandomState(seed).normal(size=ACC_N)
    x[(phi + 0.3) % 1.0 < ACC_DUCY] += amplitude
    return x.astype(np.float32)


def near_signal(freqs):
    return np.abs(np.asarray(freqs) - 1.0 / ACC_PERIOD) <= ACC_RADIUS / ACC_TOBS
