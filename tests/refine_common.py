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


def tables(rng, B, S, N, K, J):
    """Random tables in [0, N) whose first rows hold 0 and N - 1 side by side
    (the index n + dshift + pshift then reaches 3N - 3: the double wrap)."""
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
    return d, p


def widths_for(N):
    """{1, N - 1} and a middle one."""
    return np.unique(np.array([1, max(1, N // 3), N - 1], dtype=np.uint32))


def cube(rng, B, S, N, kind):
    if kind == "int":
        return rng.randint(-8, 9, size=(B, S, N)).astype(np.float32)
    return rng.normal(size=(B, S, N)).astype(np.float32)


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
