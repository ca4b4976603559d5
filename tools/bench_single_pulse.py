"""Time the single-pulse search (rt_single_pulse_device through
engine.single_pulse_device) on device-resident, normalised series: by default
16 DM trials of 2^23 samples at the default widths up to 512, radius 512,
threshold 8, Gaussian noise with a few pulses.  Between two HIP events per call
(the three launches and the read-back of the event count; the event and
workspace allocations come from torch's caching allocator, warm after the first
call); two warm-ups, then the median of --repeats calls.

Beside it:
  read_GBps   the series' bytes (read once, halos not counted) over the time,
              and its fraction of the 8 TB/s HBM peak
  host_spec   rt_single_pulse_host on one core, timed on one series of
              --host-samples samples and scaled to the job
A record, not a gate: prints one JSON line and writes it to --out.

    python tools/bench_single_pulse.py --out profiles/pulse_16x8388608.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--trials", type=int, default=16)
    ap.add_argument("--samples", type=int, default=1 << 23)
    ap.add_argument("--wmax", type=int, default=512)
    ap.add_argument("--threshold", type=float, default=8.0)
    ap.add_argument("--host-samples", type=int, default=1 << 20)
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")
    import torch
    from riptide_amd import engine
    from riptide_amd.single_pulse import events_to_host, generate_pulse_widths, single_pulse_host
    B, N = args.trials, args.samples
    widths = generate_pulse_widths(args.wmax)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    x = torch.randn((B, N), dtype=torch.float32, device=dev, generator=gen)
    for i, (w, a) in enumerate(((1, 12.0), (8, 5.0), (40, 2.0), (300, 0.8))):
        t0 = (i + 1) * (N // 5)
        x[i % B, t0:t0 + w] += a

    def call():
        return engine.single_pulse_device(x, widths, args.threshold)
    for _ in range(2):
        ev = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ev = call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    events = events_to_host(ev)

    # one-core specification on the head of the first series
    hn = max(int(widths[-1]), min(args.host_samples, N))
    head = x[0, :hn].cpu().numpy()
    t0 = time.perf_counter()
    host = single_pulse_host(head, widths, args.threshold)
    host_ms = (time.perf_counter() - t0) * 1e3 * (B * N / float(hn))
    # the device's events of that stretch, away from its cut end, are the specification's
    edge = hn - 2 * int(widths[-1])
    dev_head = events[(events["series"] == 0) & (events["sample"] < edge)]
    same = bool(np.array_equal(dev_head, host[host["sample"] < edge]))

    read_bytes = 4.0 * B * N
    result = {
        "kind": "single_pulse", "trials": B, "samples": N, "widths": int(widths.size), "wmax": int(widths[-1]),
        "radius": int(widths[-1]), "threshold": args.threshold, "tile": engine.PULSE_TILE,
        "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
        "device_ms": ms, "device_ms_min": float(min(times)), "device_ms_max": float(max(times)),
        "events": int(events.size), "read_bytes": read_bytes, "read_GBps": read_bytes / (ms * 1e-3) / 1e9,
        "fraction_of_hbm_peak": read_bytes / (ms * 1e-3) / HBM_PEAK_BPS,
        "Gsample_widths_per_s": B * N * float(widths.size) / (ms * 1e-3) / 1e9,
        "host_spec_ms_one_core": host_ms, "host_samples_timed": hn, "speedup_vs_host_spec": host_ms / ms,
        "device_events_equal_host_spec": same,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
