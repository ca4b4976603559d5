"""Time harmonic flagging (harmonic_testing.flag_harmonics: the device pair
test plus the host resolve) at N = 1024 and 4096 synthetic clusters, next to
the host loop over htest timed in the same run on a 512-cluster subset.
Reports seconds per call, nanoseconds per pair (N (N - 1) / 2 pairs, the
loop's own count for the subset) and the pair kernel's share of the C call
(HIP events around the kernel launches over the wall time of
rt_flag_harmonics).  Median of --repeats after a warm-up.  A record, not a
gate: prints one JSON line and writes it to --out.

    python tools/bench_harmonics.py --out profiles/<tag>_harmonics.json
"""
import argparse
import ctypes
import json
import os
import sys
import time
from collections import namedtuple

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TOBS, FMIN, FMAX = 540.0, 1200.0, 1500.0
Centre = namedtuple("Centre", "freq snr ducy dm")


def synthetic(n, seed=0):
    """Periods 0.1-10 s, S/N 7-60, ducy width / 240-260 bins, DMs on a 0.1
    grid; every sixth cluster has a 2nd or 3rd harmonic planted."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        c = Centre(1.0 / rng.uniform(0.1, 10.0), float(rng.uniform(7.0, 60.0)),
                   float(rng.choice([1, 2, 3, 4, 6, 9, 13, 19, 28, 42])) / float(rng.randint(240, 261)),
                   round(rng.uniform(0.0, 100.0) * 10) / 10.0)
        out.append(c)
        if len(out) % 6 == 0:
            k = 2 + len(out) % 2
            out.append(Centre(c.freq * k * (1.0 + rng.uniform(-2e-6, 2e-6)),
                              c.snr / k ** 0.5 + rng.uniform(-2.5, 2.5), c.ducy, c.dm))
    return out[:n]


def median_seconds(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bench
    import riptide_amd
    from riptide_amd import _lib, harmonic_testing as ht

    lib = _lib.load()
    result = {"tobs": TOBS, "fmin": FMIN, "fmax": FMAX, "denom_max": 100, "repeats": args.repeats,
              "source_digest": bench.source_digest(), "device": torch.cuda.get_device_name(0)}

    def clusters_of(centres):
        return [riptide_amd.PeakCluster([c]) for c in centres]

    # the host loop over htest, the reference's way
    sub = synthetic(512)
    host = clusters_of(sub)
    ordered = sorted(host, key=lambda c: c.centre.snr, reverse=True)
    tested = 0
    t0 = time.perf_counter()
    for i, F in enumerate(ordered):
        for H in ordered[i + 1:]:
            if F.is_harmonic or H.is_harmonic:
                continue
            tested += 1
            related, fraction = ht.htest(F.centre, H.centre, TOBS, FMIN, FMAX)
            if related:
                H.parent_fundamental, H.hfrac = F, fraction
    t_host = time.perf_counter() - t0
    dev = clusters_of(sub)
    riptide_amd.flag_harmonics(dev, TOBS, FMIN, FMAX)
    same = all((a.parent_fundamental is None) == (b.parent_fundamental is None) and a.hfrac == b.hfrac
               for a, b in zip(host, dev))
    assert same, "flag_harmonics differs from the host loop"
    result["host_loop_512"] = {"seconds": t_host, "pairs_tested": int(tested),
                               "ns_per_tested_pair": 1e9 * t_host / tested,
                               "flagged": sum(c.is_harmonic for c in host)}

    for n in (1024, 4096):
        centres = synthetic(n)
        pairs = n * (n - 1) // 2

        def call():
            riptide_amd.flag_harmonics(clusters_of(centres), TOBS, FMIN, FMAX)

        t_py = median_seconds(call, args.repeats)
        # the C call alone, on prepared arrays
        ranked = sorted(centres, key=lambda c: c.snr, reverse=True)
        cols = ht._columns(ranked)
        prm = ht._params(TOBS, FMIN, FMAX, 100)
        parent, hnum, hden = np.empty(n, np.int32), np.empty(n, np.int64), np.empty(n, np.int64)

        def c_call():
            rc = lib.rt_flag_harmonics(*(_lib.ptr(c) for c in cols), n, ctypes.addressof(prm), 0, _lib.ptr(parent),
                                       _lib.ptr(hnum), _lib.ptr(hden))
            assert rc == 0

        t_c = median_seconds(c_call, args.repeats)
        tiles, near, rows = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        ms = ctypes.c_double()
        lib.rt_flag_harmonics_stats(ctypes.byref(tiles), ctypes.byref(near), ctypes.byref(rows), ctypes.byref(ms))
        result[f"n{n}"] = {"pairs": pairs, "flag_harmonics_s": t_py, "ns_per_pair": 1e9 * t_py / pairs,
                           "c_call_s": t_c, "c_ns_per_pair": 1e9 * t_c / pairs, "kernel_ms": ms.value,
                           "kernel_share_of_c_call": ms.value * 1e-3 / t_c, "tiles": tiles.value,
                           "near_pairs": near.value, "host_rows": rows.value,
                           "flagged": int(np.count_nonzero(parent >= 0))}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
