"""Time the acceleration search's resampling (rt_resample_device through
engine.resample_device) on device-resident series: N = 2^23 samples, R = 8, 32
and 128 output rows drawn from 8 sources with factors spread over +-0.5 / N.
Between two HIP events per call, after two warm-ups, the median of --repeats
calls.

Beside it:
  GBps         the algorithmic 8 * N bytes per row (one read, one write) over
               the time, and its fraction of the 8 TB/s HBM peak
  torch_*      the same gather by torch.take_along_dim on the gathered source
               rows with precomputed int64 indices (an outside yardstick: it
               also reads 8 bytes of index per output, and is handed the
               source rows already expanded to [R, N]); the outputs are
               compared bit for bit
  search       EngineSearcher.search_device_accel of --series series of
               --search-samples samples with --accels trial accelerations,
               against as many plain search_device calls (which normalise again
               and do not resample): host clock around a synchronise
A record, not a gate: prints one JSON line and writes it to --out.

    python tools/bench_resample.py --out profiles/ac01a_resample.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_BPS = 8.0e12
RANGES = [{"name": "bench", "ffa_search": {"period_min": 0.5, "period_max": 2.0, "bins_min": 240, "bins_max": 260},
           "find_peaks": {"smin": 7.0}}]
DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}


def timed(torch, call, repeats):
    for _ in range(2):
        out = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return out, float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--samples", type=int, default=1 << 23)
    ap.add_argument("--rows", type=int, nargs="+", default=[8, 32, 128])
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--series", type=int, default=8)
    ap.add_argument("--search-samples", type=int, default=1 << 20)
    ap.add_argument("--accels", type=int, default=5)
    ap.add_argument("--search-repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    from riptide_amd import engine
    from riptide_amd.dispatch import EngineSearcher
    B, N = args.sources, args.samples
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    x = torch.randn((B, N), dtype=torch.float32, device=dev, generator=gen)
    result = {"kind": "resample", "samples": N, "sources": B, "device": torch.cuda.get_device_name(0),
              "repeats": args.repeats, "rows": []}
    for R in args.rows:
        src = (np.arange(R) * 3 % B).astype(np.int32)
        f = np.linspace(-0.5, 0.5, R) / N
        out, ms, lo, hi = timed(torch, lambda: engine.resample_device(x, f, src=src), args.repeats)
        # the yardstick's inputs, built on the device: torch.round is half-even, as rint
        j = torch.arange(N, dtype=torch.int64, device=dev)
        q = (j * (N - j)).double()
        idx = torch.stack([(j - torch.round(float(v) * q).long()).clamp_(0, N - 1) for v in f])
        xs = x[torch.from_numpy(src.astype(np.int64)).to(dev)]
        tout, tms, tlo, thi = timed(torch, lambda: torch.take_along_dim(xs, idx, dim=1), args.repeats)
        same = bool(torch.equal(out.view(torch.int32), tout.view(torch.int32)))
        alg = 8.0 * N * R
        result["rows"].append({
            "rows": R, "ms": ms, "ms_min": lo, "ms_max": hi, "alg_bytes": alg, "GBps": alg / (ms * 1e-3) / 1e9,
            "fraction_of_hbm_peak": alg / (ms * 1e-3) / HBM_PEAK_BPS,
            "torch_ms": tms, "torch_ms_min": tlo, "torch_ms_max": thi, "torch_GBps": alg / (tms * 1e-3) / 1e9,
            "torch_over_kernel": tms / ms, "equal_bits": same})
        del idx, xs, out, tout

    # the search: A trial accelerations against A plain searches of the same series
    D, n, A, tsamp = args.series, args.search_samples, args.accels, 256e-6
    raw = torch.randn((D, n), dtype=torch.float32, device=dev, generator=gen)
    metas = [{"dm": float(k)} for k in range(D)]
    tobs = n * tsamp
    amax = 0.25 / n * 2 * 299792458.0 / tsamp             # |f| * N = 0.25 at the ends of the grid
    accels = np.linspace(-amax, amax, A).tolist()
    searcher = EngineSearcher(DEREDDEN, RANGES, device=0, batch=8)

    def wall(call):
        call()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.search_repeats):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times))
    accel_ms = wall(lambda: searcher.search_device_accel(raw, tsamp, metas, accels))
    plain_ms = wall(lambda: [searcher.search_device(raw, tsamp, metas) for _ in range(A)])
    result["search"] = {"series": D, "samples": n, "tsamp": tsamp, "tobs": tobs, "accels": A, "batch": searcher.batch,
                        "repeats": args.search_repeats, "search_device_accel_ms": accel_ms,
                        "plain_search_device_x_accels_ms": plain_ms, "accel_over_plain": accel_ms / plain_ms,
                        "dm_accel_trials_per_s": D * A / (accel_ms * 1e-3)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
