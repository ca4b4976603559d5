"""Time the pulse cutouts (rt_pulse_cutouts_device through
engine.pulse_cutouts_device) on a device-resident block: by default 1024
channels of 8-bit noise, 2^16 rows, and the frequency-time and DM-time cutouts
of 256 pulses (pulse_candidates.cutout_jobs at its defaults: 256 bins, 64
bands, 64 DMs, so 128 jobs per pulse) of widths 1 to 128 samples spread over
the block.  Between two HIP events per call (the job table's upload, the
transpose of the block and the one cutout launch; the output and workspace come
from the caller, warm); two warm-ups, then the median of --repeats calls.

Beside it:
  host_spec   rt_pulse_cutouts_host on one core, timed on the jobs of the
              first --host-pulses pulses and scaled to the job by the samples
              summed (nbins * factor * channels per job)
  equal       whether the device's floats of those pulses are the host's bits
A record, not a gate: prints one JSON line and writes it to --out.

    python tools/bench_pulse_cutouts.py --out profiles/pulse_cutouts_1024x65536.json
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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--nchans", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=1 << 16)
    ap.add_argument("--pulses", type=int, default=256)
    ap.add_argument("--host-pulses", type=int, default=4)
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")
    import torch
    from riptide_amd import engine
    from riptide_amd import pulse_candidates as pc
    from riptide_amd.single_pulse import SinglePulse
    C, N, P = args.nchans, args.samples, args.pulses
    rng = np.random.RandomState(0)
    x = np.clip(np.round(rng.normal(100.0, 10.0, size=(N, C))), 0, 255).astype(np.uint8)
    freqs = 1500.0 - 300.0 / C * np.arange(C)
    tsamp = 256e-6
    widths = [1, 2, 4, 8, 16, 32, 64, 128]
    pulses = [SinglePulse(0.0, int(rng.randint(N // 8, N - N // 8)), float(rng.uniform(5.0, 80.0)), 0,
                          widths[i % len(widths)], 10.0, 1, 0.0, 0.0) for i in range(P)]
    plan = pc.cutout_jobs(pulses, freqs, tsamp)
    jobs = plan.jobs
    work = jobs["nbins"].astype(np.float64) * jobs["factor"] * (jobs["band_hi"] - jobs["band_lo"])

    dev = torch.device("cuda", 0)
    block = torch.from_numpy(x).to(dev)
    delays = torch.from_numpy(plan.delays).to(dev)
    out = torch.empty(int((jobs["out_off"] + jobs["nbins"]).max()), dtype=torch.float32, device=dev)
    ws = torch.empty(engine.dedisperse_workspace_bytes("uint8", N, C), dtype=torch.uint8, device=dev)

    def call():
        return engine.pulse_cutouts_device(block, jobs, delays, plan.max_delay, out=out, workspace=ws)
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    got = out.cpu().numpy()

    # one-core specification on the first pulses' jobs, scaled by the samples summed
    hp = max(1, min(args.host_pulses, P))
    nj = hp * plan.rows_per_pulse
    t0 = time.perf_counter()
    host = pc.pulse_cutouts_host(x, jobs[:nj], plan.delays, plan.max_delay)
    host_s = time.perf_counter() - t0
    host_ms = host_s * 1e3 * float(work.sum() / work[:nj].sum())
    same = bool(np.array_equal(got[:host.size].view(np.uint32), host.view(np.uint32)))

    result = {
        "kind": "pulse_cutouts", "nchans": C, "samples": N, "dtype": "uint8", "pulses": P, "jobs": int(jobs.size),
        "nbins": plan.nbins, "nbands": plan.nbands, "ndm": plan.ndm, "factors": sorted(set(int(f) for f in plan.factors)),
        "tile": engine.pulse_cutouts_plan(1, 0, 4)[0],
        "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
        "device_ms": ms, "device_ms_min": float(min(times)), "device_ms_max": float(max(times)),
        "samples_summed": float(work.sum()), "Gsamples_per_s": float(work.sum()) / (ms * 1e-3) / 1e9,
        "host_spec_ms_one_core": host_ms, "host_pulses_timed": hp, "host_seconds_timed": host_s,
        "speedup_vs_host_spec": host_ms / ms, "device_equal_host_spec": same,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
