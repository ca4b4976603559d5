#!/usr/bin/env python3
"""Device vs host find_peaks on cfg2 periodograms (GPU box):
ms per trial of PeakFinder (HIP order statistics + threshold selection, host
polyfit/cluster) and of the reference-restated numpy find_peaks.

--ab: PeakFinder.__call__ with device_cluster off and on at the same commit:
wall time (median of --repeats after a warm-up, a device synchronise inside
the window) and device->host copies per call (Tensor.cpu calls), on cfg5's
three ranges at B = 16 noise trials and on a "bright" case (the short range,
a pulsar of S/N about 50 in every trial).  The peaks are asserted equal
before timing.  --out writes the JSON record."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


CFG5_N, CFG5_TSAMP = 1 << 23, 64e-6
CFG5_RANGES = (("short", 0.2, 0.5, 240, 260), ("medium", 0.5, 2.0, 480, 520), ("long", 2.0, 120.0, 960, 1040))


def ab(repeats, out):
    import statistics
    import numpy as np
    import torch
    from riptide_amd import engine
    from riptide_amd.libffa import generate_signal
    from riptide_amd.peaks import PeakFinder
    n, tsamp, B = CFG5_N, CFG5_TSAMP, 16
    copies = {"n": 0}
    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        copies["n"] += 1
        return real_cpu(self, *a, **k)

    def timed(finder, snr, dms):
        finder(snr, dms=dms)
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            finder(snr, dms=dms)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        torch.Tensor.cpu = counting_cpu
        copies["n"] = 0
        try:
            finder(snr, dms=dms)
        finally:
            torch.Tensor.cpu = real_cpu
        return {"ms_median": statistics.median(times), "ms_all": times, "d2h_copies": copies["n"]}

    gen = torch.Generator(device="cuda").manual_seed(1)
    noise = torch.randn((B, n), device="cuda", dtype=torch.float32, generator=gen)
    np.random.seed(2)
    # amplitude = the S/N of the folded profile (unit-norm pulse train, unit noise)
    pulse = torch.from_numpy(np.asarray(generate_signal(n, 0.3141 / tsamp, ducy=0.03, amplitude=50.0, stdnoise=0.0),
                                        dtype=np.float32)).cuda()
    cases = [(name, noise, r) for name, *r in CFG5_RANGES] + [("bright_short", noise + pulse, CFG5_RANGES[0][1:])]
    dms = [float(b) for b in range(B)]
    result = {"batch": B, "n": n, "tsamp": tsamp, "repeats": repeats, "cases": {}}
    for name, x, (pmin, pmax, bmin, bmax) in cases:
        plan = engine.PeriodogramPlan.for_search(n, tsamp, pmin, pmax, bmin, bmax, wtsp=1.5)
        snr = plan.run(x)
        off, on = PeakFinder(plan, n * tsamp), PeakFinder(plan, n * tsamp, device_cluster=True)
        a, b = off(snr, dms=dms), on(snr, dms=dms)
        assert [p for p, _ in a] == [p for p, _ in b], f"{name}: device_cluster changes the peaks"
        assert all(np.array_equal(pa[iw], pb[iw]) for (_, pa), (_, pb) in zip(a, b) for iw in pa)
        sel = int(((snr > 6.0).sum()).item())
        result["cases"][name] = {"L": int(snr.shape[1]), "W": int(snr.shape[2]), "rows_above_smin": sel,
                                 "peaks": sum(len(p) for p, _ in a), "off": timed(off, snr, dms),
                                 "on": timed(on, snr, dms)}
        del snr, plan
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="store_true", help="device_cluster off against on (cfg5 ranges, B = 16)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.ab:
        return ab(args.repeats, args.out)
    import numpy as np
    import torch
    from riptide_amd import engine
    from riptide_amd.metadata import Metadata
    from riptide_amd.peak_detection import find_peaks
    from riptide_amd.peaks import PeakFinder
    from riptide_amd.periodogram import Periodogram
    n, tsamp, B = 1 << 23, 256e-6, 8
    plan = engine.PeriodogramPlan.for_search(n, tsamp, 0.1, 10.0, 240, 260, ducy_max=0.05)
    x = torch.randn((B, n), device="cuda", dtype=torch.float32)
    snr = plan.run(x)
    finder = PeakFinder(plan, n * tsamp)
    finder(snr, dms=[0.0] * B)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        res = finder(snr, dms=[0.0] * B)
    torch.cuda.synchronize()
    dev_ms = (time.perf_counter() - t0) / (3 * B) * 1e3
    periods, foldbins = plan.grid()
    s0 = snr[0].cpu().numpy()
    t0 = time.perf_counter()
    pg = Periodogram(plan.widths, periods, foldbins, s0, metadata=Metadata({"tobs": n * tsamp, "dm": 0.0}))
    ref, _ = find_peaks(pg)
    host_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"device_ms_per_trial": dev_ms, "host_ms_per_trial": host_ms, "peaks_trial0": len(res[0][0]),
                      "identical_trial0": res[0][0] == ref, "nseg": finder.nseg, "per_seg": finder.per_seg}))


if __name__ == "__main__":
    main()
