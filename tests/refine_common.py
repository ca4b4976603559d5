"""Shared by test_refine_host.py and test_gpu_refine.py: numpy restatements of
the refinement's shift tables and profiles, the test cubes and tables, and the
recovery case."""
import numpy as np

KDM = 1.0 / 2.41e-4


def numpy_shifts(P, T, N, S, f, dm, kdm, periods, dms):
    """The two formulas of rt_refine_shifts in float64, in the operation
    order its header states."""
    f = np.asarray(f, dtype=np.float64)
    periods = np.asarray(periods, dtype=np.float64)
    dms = np.asarray(dms, dtype=np.float64)
    a = 1.0 / P - 1.0 / periods
    c = (np.arange(S, dtype=np.float64) + 0.5) / float(S) - 0.5
    vp = np.floor(float(N) * T * a[:, None] * c[None, :] + 0.5)
    fmax = f.max()
    g = 1.0 / (f * f) - 1.0 / (fmax * fmax)
    vd = np.floor(float(N) * kdm * (dms - dm)[:, None] * g[None, :] / P + 0.5)
    return np.mod(vp, float(N)).astype(np.int32), np.mod(vd, float(N)).astype(np.int32), vp, vd


def numpy_profiles(x, dshift, pshift):
    """prof [K, J, N] in float64 (roll and sum), and the sum of the terms'
    magnitudes for the float bound."""
    x = np.asarray(x, dtype=np.float64)
    B, S, N = x.shape
    n = np.arange(N)
    K, J = dshift.shape[0], pshift.shape[0]
    prof = np.zeros((K, J, N))
    mag = np.zeros((K, J, N))
    for k in range(K):
        for j in range(J):
            idx = (n[None, None, :] + dshift[k].astype(np.int64)[:, None, None]
                   + pshift[j].astype(np.int64)[None, :, None]) % N
            t = np.take_along_axis(x, idx, axis=2)
            prof[k, j] = t.sum(axis=(0, 1))
            mag[k, j] = np.abs(t).sum(axis=(0, 1))
    return prof, mag


CHUNK = 256     # rows of shifts the kernels load at a time (kRefineThreads)


def _chunked_table(rng, t, N):
    """A table of more than CHUNK rows per trial: every trial random, so that
    no chunk of a trial repeats another (a constant trial would hide a chunk
    read twice or from the wrong buffer), with N - 1 and 0 side by side in the
    middle of the first trial, at the start of the last, and in every trial
    across the first chunk boundary (rows CHUNK - 1 and CHUNK).  Every other
    entry differs from the entries CHUNK, 2 CHUNK, ... rows away."""
    T, R = t.shape
    assert R > CHUNK and N > 2 * ((R - 1) // CHUNK + 1)
    t[0] = rng.randint(0, N, size=R)
    t[-1] = rng.randint(0, N, size=R)
    planted = np.zeros(t.shape, dtype=bool)
    for row, at in ((0, R // 2 - 1), (T - 1, 0)) + tuple((i, CHUNK - 1) for i in range(T)):
        t[row, at:at + 2] = [N - 1, 0]
        planted[row, at:at + 2] = True
    for i in range(T):
        for r in range(R):
            others = [t[i, q] for q in range(r % CHUNK, R, CHUNK) if q != r]
            while not planted[i, r] and t[i, r] in others:
                t[i, r] = (t[i, r] + 1) % N
    return t


def tables(rng, B, S, N, K, J):
    """Random tables in [0, N) whose first rows hold 0 and N - 1 side by side
    (the index n + dshift + pshift then reaches 3N - 3: the double wrap).  A
    table of more than CHUNK rows is _chunked_table's."""
    d = rng.randint(0, N, size=(K, B)).astype(np.int32)
    p = rng.randint(0, N, size=(J, S)).astype(np.int32)
    d[0, :] = N - 1
    p[0, :] = N - 1
    d[0, B // 2] = 0
    p[0, S // 2] = 0
    if K > 1:
        d[-1, :] = 0
        d[-1, 0] = N - 1
    if J > 1:
        p[-1, :] = 0
        p[-1, -1] = N - 1
    if B > CHUNK:
        _chunked_table(rng, d, N)
    if S > CHUNK:
        _chunked_table(rng, p, N)
    return d, p


def check_chunked_table(t, N):
    """What a test of more than CHUNK rows relies on (see _chunked_table)."""
    T, R = t.shape
    assert R > CHUNK
    chunks = [t[:, r0:r0 + CHUNK] for r0 in range(0, R, CHUNK)]
    for c in range(1, len(chunks)):
        for e in range(c):
            n = chunks[c].shape[1]                   # the last chunk is the shorter one
            differ = chunks[c] != chunks[e][:, :n]
            assert differ.any(axis=1).all(), (e, c)  # no two chunks of a table row are equal
            if e == c - 1:
                assert (2 * differ.sum(axis=1) >= n).all(), c
    assert list(t[0, R // 2 - 1:R // 2 + 1]) == [N - 1, 0] and list(t[-1, :2]) == [N - 1, 0]
    assert (t[:, CHUNK - 1] == N - 1).all() and (t[:, CHUNK] == 0).all()
    assert t.min() == 0 and t.max() == N - 1


def widths_for(N):
    """{1, N - 1} and a middle one."""
    return np.unique(np.array([1, max(1, N // 3), N - 1], dtype=np.uint32))


def cube(rng, B, S, N, kind):
    if kind == "int":
        return rng.randint(-8, 9, size=(B, S, N)).astype(np.float32)
    return rng.normal(size=(B, S, N)).astype(np.float32)


def job(B, S, N, K, J, kind, seed=0):
    """(cube, dshift, pshift, widths, stdnoise) of a shape: refine_host's and
    refine_many's arguments."""
    rng = np.random.RandomState(seed + B * 1000 + S * 10 + N)
    d, p = tables(rng, B, S, N, K, J)
    return (cube(rng, B, S, N, kind), d, p, widths_for(N), 1.7)


# ---- a batch of 40: eight small shapes (B, S, N, K, J) in turn, K and J in
# 1..4, among them one of a single stage-A block (S = 1) and one of a single
# stage-B block (K = 1); the first, a middle and the last candidate are one
# block in both stages, so the kernels' search for a block's candidate meets
# a one-block entry at each end of its table and inside it
BATCH_CYCLE = [(3, 2, 64, 2, 3), (5, 1, 33, 2, 3), (4, 3, 65, 1, 2), (8, 8, 100, 4, 4), (2, 5, 7, 3, 1), (7, 2, 31, 4, 2),
               (1, 4, 2, 2, 2), (6, 3, 96, 3, 4)]
BATCH_SINGLE = (2, 1, 9, 1, 1)
BATCH_SIZE = 40


def batch_shapes():
    shapes = [BATCH_CYCLE[i % len(BATCH_CYCLE)] for i in range(BATCH_SIZE)]
    for i in (0, BATCH_SIZE // 2, BATCH_SIZE - 1):
        shapes[i] = BATCH_SINGLE
    return shapes


def batch_jobs():
    """The batch's jobs: every candidate its own cube and tables."""
    return [job(*s, "normal", seed=100 + i) for i, s in enumerate(batch_shapes())]


# ---- S/N of profiles with a large offset: the last expression of refine_snr1,
# (h + b) * dmax - b * sum, is then a difference of two large terms
OFFSET = 100.0
OFFSET_SHAPES = [(8, 8, 64, 3, 3), (3, 2, 700, 2, 2)]


def offset_job(B, S, N, K, J):
    """job()'s "normal" cube plus OFFSET per cell: widths {1, N // 3, N - 1},
    stdnoise 1.7."""
    g = job(B, S, N, K, J, "normal", seed=11)
    return (g[0] + np.float32(OFFSET),) + g[1:]


def snr1_terms(prof, widths):
    """h, b [W], dmax [rows, W] and sum [rows, 1] as refine_snr1
    (refine_host.hpp) states them, every one the float32 it computes: prefix
    sums accumulated in double and rounded as stored, the wrapped part
    cps[N + i] = cps[i] + sum in float32, float32 differences."""
    prof = np.asarray(prof, dtype=np.float32)
    N = prof.shape[-1]
    prof = prof.reshape(-1, N)
    cps = np.cumsum(prof.astype(np.float64), axis=1).astype(np.float32)
    total = cps[:, -1:]
    ext = np.concatenate([cps, cps + total], axis=1)
    assert ext.dtype == np.float32
    h, b, dmax = [], [], []
    for w in (int(w) for w in widths):
        hw = np.sqrt(np.float32(N - w) / np.float32(N * w))
        h.append(hw)
        b.append(np.float32(w) / np.float32(N - w) * hw)
        dmax.append((ext[:, w:w + N] - ext[:, :N]).max(axis=1))
    h, b, dmax = np.array(h), np.array(b), np.stack(dmax, axis=1)
    assert h.dtype == b.dtype == dmax.dtype == np.float32
    return h, b, dmax, total


def snr1_bound(prof, widths, stdnoise):
    """(the float32 evaluation of refine_snr1's last expression, its float64
    evaluation from the same float32 terms, the bound on a float32
    evaluation's distance from either), each [rows, W].  The float32
    expression rounds h + b, two products, a difference and a quotient: half
    an ulp each of a value no larger than |h + b| |dmax| + |b| |sum| before
    the division, 2.5 * 2^-24 of that in all.  A fused multiply-add drops one
    of the roundings; a square root or a division of h and b that is one ulp
    off moves each product by 2^-23 of itself.  8 * 2^-24 covers all of
    these together."""
    h, b, dmax, total = snr1_terms(prof, widths)
    sd = np.float32(stdnoise)
    f32 = ((h + b) * dmax - b * total) / sd
    assert f32.dtype == np.float32
    h, b, dmax, total, sd = (np.asarray(v, dtype=np.float64) for v in (h, b, dmax, total, sd))
    f64 = ((h + b) * dmax - b * total) / sd
    bound = 8 * 2.0 ** -24 * (np.abs(h + b) * np.abs(dmax) + np.abs(b) * np.abs(total)) / sd
    return f32, f64, bound


# ---- recovery: a pulse that only the trial (RK, RJ) lines up
RB, RS, RN, RTRIALS = 8, 8, 64, 9
RK, RJ = 6, 2                   # off the centre (4, 4)
R_PERIOD, R_DM, R_N0, R_WIDTH = 0.5, 30.0, 20, 4
R_TOBS = 600 * R_PERIOD
R_FREQS = np.array([1500.0, 1462.0, 1431.0, 1388.0, 1350.0, 1321.0, 1270.0, 1233.0])
# The pulse's height in every (band, sub-integration), in units of the noise
# sigma.  Lined up, the 64 rows give a 4-bin pulse of 64 * 1.5 over a bin noise
# of 8: S/N about 24.  A neighbouring trial moves a few of the rows by one bin
# and shares every other sample, so its S/N is lower by the moved rows' share
# while its noise is almost the same.  With the host specification over seeds
# 0..19 (test_recovery_host): 0.75 recovers the trial on 18 seeds, 1.0 on all 20
# with the runner-up 0.24 behind, 1.5 on all 20 with the runner-up 0.75 behind.
R_AMPLITUDE = 1.5
R_WIDTHS = np.array([1, 2, 3, 4, 6, 9, 12], dtype=np.uint32)


def recovery_trials():
    """(periods [9], dms [9]): one bin of drift over the span, one bin of
    delay at the lowest band, per step, centred on the fold's values."""
    j = np.arange(RTRIALS) - RTRIALS // 2
    periods = 1.0 / (1.0 / R_PERIOD - j / (RN * R_TOBS))
    span = R_FREQS.min() ** -2.0 - R_FREQS.max() ** -2.0
    dms = R_DM + j * R_PERIOD / (RN * KDM * span)
    return periods, dms


def recovery_cube(seed, pshift, dshift):
    """Noise of sigma 1 plus a boxcar pulse at (R_N0 + dshift[RK][b] +
    pshift[RJ][s]) mod N: the definition reads x[b][s][(n + dshift + pshift) mod
    N], so trial (RK, RJ), and no other, brings every row's pulse to R_N0.  (With
    the shifts subtracted the mirrored trial (8 - RK, 8 - RJ) would line up.)"""
    rng = np.random.RandomState(seed)
    x = rng.normal(size=(RB, RS, RN))
    for b in range(RB):
        for s in range(RS):
            at = (R_N0 + int(dshift[RK, b]) + int(pshift[RJ, s]) + np.arange(R_WIDTH)) % RN
            x[b, s, at] += R_AMPLITUDE
    return x.astype(np.float32)
