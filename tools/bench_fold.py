"""Time the batched candidate fold (folding.fold_many) against the
per-candidate loop of folding.fold: 32 candidates of one 2^23-sample series,
periods 0.1-10 s, 128 bins, with 32 sub-integrations (vertical mode) and with
one (profile mode).  Median of 5 after a warm-up; next to it the time of the
device-resident call (engine.fold_device on a resident series, between two
HIP events: spec packing, the two allocations, the table copy and both
kernels -- not the kernels alone).  A record, not a gate: prints one JSON line and writes
it to --out.

    python tools/bench_fold.py --out profiles/<tag>_fold_many.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


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
    from riptide_amd import engine
    from riptide_amd.folding import fold, fold_many

    n, tsamp, bins, ncand = 1 << 23, 256e-6, 128, 32
    data = np.random.RandomState(0).normal(size=n).astype(np.float32)
    ts = riptide_amd.TimeSeries.from_numpy_array(data, tsamp)
    periods = np.geomspace(0.1, 10.0, ncand)
    dev = torch.from_numpy(data).cuda()
    result = {"samples": n, "tsamp": tsamp, "bins": bins, "candidates": ncand, "repeats": args.repeats,
              "source_digest": bench.source_digest(), "device": torch.cuda.get_device_name(0)}
    for name, subints in (("subints32", 32), ("profile", 1)):
        specs = [(float(p), bins, subints) for p in periods]
        many = fold_many(ts, specs)
        loop = [fold(ts, *s) for s in specs]
        assert all(np.array_equal(a, b) for a, b in zip(many, loop)), "fold_many differs from the fold loop"
        t_many = median_seconds(lambda: fold_many(ts, specs), args.repeats)
        t_loop = median_seconds(lambda: [fold(ts, *s) for s in specs], args.repeats)
        dspecs = [(0,) + s for s in specs]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        engine.fold_device(dev, tsamp, dspecs)
        ms = []
        for _ in range(args.repeats):
            a.record()
            engine.fold_device(dev, tsamp, dspecs)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        result[name] = {"fold_many_s": t_many, "fold_loop_s": t_loop, "speedup": t_loop / t_many,
                        "fold_device_call_ms": float(np.median(ms))}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
