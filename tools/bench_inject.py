"""Time the signal injection (rt_inject_device through engine.inject_device) on
one device-resident uint8 block of --chans x --samples (default 1024 x 2^22,
4 GiB): K = 1, 4 and 16 periodic signals, without and with acceleration;
beside it a device-to-device copy of the same block, the bandwidth yardstick
(one read and one write of every byte, what the injection also moves), and
the host specification (injection.inject_host) on the first --host-samples
rows (one warm-up call, the median of --rounds more), scaled to the block by
the row count.

Host clock around a device synchronise; one warm-up round, then --rounds
rounds that alternate between all device cases, so a drift of the clocks
falls on every case alike; median [min, max] per case.  A record, not a gate:
prints one JSON line and writes it to --out.

    python tools/bench_inject.py --out profiles/in01a_inject.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--chans", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=1 << 22)
    ap.add_argument("--signals", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-samples", type=int, default=1 << 12)
    args = ap.parse_args()
    import torch
    from riptide_amd import engine
    from riptide_amd.injection import PulsarSignal, inject_host, injection_tables
    n, g, tsamp = args.chans, args.samples, 64e-6
    dev = torch.device("cuda", 0)
    freqs = 1500.0 - np.arange(n) * (300.0 / n)
    span = min(g, 1 << 27)
    block = torch.randint(0, 256, (g, n), dtype=torch.uint8, device=dev)
    spare = torch.empty_like(block)
    amax = 0.25 / span * 2 * 299792458.0 / tsamp            # |f| * span = 0.25

    def tables(K, accel):
        sig = [PulsarSignal(0.05 + 0.013 * k, 20.0 + 5.0 * k, 15.0, accel=amax * (k + 1) / K if accel else 0.0)
               for k in range(K)]
        return injection_tables(sig, freqs, tsamp, span, 10.0)

    cases = {"copy": lambda: spare.copy_(block)}
    for K in args.signals:
        for accel in (False, True):
            T = tables(K, accel)
            cases[f"K{K}{'_accel' if accel else ''}"] = lambda T=T: engine.inject_device(block, T, 0, 1)
    times = {name: [] for name in cases}
    for rnd in range(args.rounds + 1):
        for name, call in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3)
    result = {"kind": "inject", "chans": n, "samples": g, "dtype": "uint8", "device": torch.cuda.get_device_name(0),
              "rounds": args.rounds, "bytes_moved": 2.0 * g * n, "cases": {}}
    copy_ms = float(np.median(times["copy"]))
    for name, t in times.items():
        ms = float(np.median(t))
        result["cases"][name] = {"ms": ms, "ms_min": float(min(t)), "ms_max": float(max(t)),
                                 "GBps": 2.0 * g * n / (ms * 1e-3) / 1e9, "over_copy": ms / copy_ms}
    # the host specification on the first rows, scaled to the block
    hg = min(args.host_samples, g)
    x = block[:hg].cpu().numpy()
    result["host"] = {}
    for K in args.signals:
        T = tables(K, False)
        t = []
        for rnd in range(args.rounds + 1):       # one warm-up, as the device cases
            t0 = time.perf_counter()
            inject_host(x, T, 0, 1)
            if rnd:
                t.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(t))
        result["host"][f"K{K}"] = {"samples": hg, "ms": ms, "ms_min": float(min(t)), "ms_max": float(max(t)),
                                   "ms_scaled_to_block": ms * g / hg}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
