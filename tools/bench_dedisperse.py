"""Time the dedispersion kernels (engine.dedisperse_device) on one resident
block of synthetic uint8 data generated on the device: by default 1024
channels x 2^22 samples at 256 DMs of a 1.2-1.5 GHz band sampled at 256 us.
Between two HIP events per call (transpose + shift-and-add, output and
workspace preallocated); one warm-up, then the median of --repeats calls.

Reports ms per DM trial, channel-samples/s, algorithmic bytes/s (block read
once, output written once) and the ratio of the per-trial time to the
per-trial search time of BENCH_r06.json (cfg2: ms_per_step over 16 trials).
A record, not a gate: prints one JSON line and writes it to --out.

    python tools/bench_dedisperse.py --out profiles/<tag>_dedisperse.json
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--nchans", type=int, default=1024)
    ap.add_argument("--log2-nsamp", type=int, default=22)
    ap.add_argument("--ndm", type=int, default=256)
    ap.add_argument("--dm-max", type=float, default=255.0)
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")
    import torch
    import bench
    from riptide_amd import engine
    from riptide_amd.dedispersion import dispersion_delays

    nchans, nsamp, ndm, tsamp = args.nchans, 1 << args.log2_nsamp, args.ndm, 256e-6
    freqs = 1500.0 - (300.0 / nchans) * np.arange(nchans)
    dms = np.linspace(0.0, args.dm_max, ndm)
    delays, max_delay = dispersion_delays(freqs, dms, tsamp)
    nout = nsamp - max_delay
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    block = torch.randint(0, 256, (nsamp, nchans), dtype=torch.uint8, device="cuda", generator=gen)
    d_delays = torch.from_numpy(delays.astype(np.int32)).cuda()
    out = torch.empty((ndm, nout), dtype=torch.float32, device="cuda")
    ws = torch.empty(engine.dedisperse_workspace_bytes("uint8", nsamp, nchans), dtype=torch.uint8, device="cuda")

    def run():
        engine.dedisperse_device(block, d_delays, max_delay, out=out, workspace=ws)

    run()
    torch.cuda.synchronize()
    # spot check of the warm-up's result against the definition: 4 DMs x 64 outputs
    rows = [0, ndm // 3, ndm // 2, ndm - 1]
    t_chk = min(12345, nout - 64)
    times = torch.arange(t_chk, t_chk + 64, device="cuda")
    idx = torch.from_numpy(delays[rows]).cuda()[:, None, :] + times[None, :, None]
    ref = block[idx, torch.arange(nchans, device="cuda")[None, None, :]].to(torch.int64).sum(dim=2)
    got = out[rows, t_chk:t_chk + 64].to(torch.int64)
    assert torch.equal(got, ref), "dedisperse_device differs from its definition"
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(args.repeats):
        a.record()
        run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    with open(os.path.join(REPO, "BENCH_r06.json")) as f:
        search_ms = json.load(f)["parsed"]["ms_per_step"] / 16.0
    result = {"nchans": nchans, "nsamp": nsamp, "ndm": ndm, "tsamp": tsamp, "dm_max": float(dms[-1]),
              "max_delay": max_delay, "nout": nout, "dtype": "uint8", "repeats": args.repeats,
              "call_ms_median": med, "call_ms_min": float(np.min(ms)), "call_ms_max": float(np.max(ms)),
              "ms_per_dm_trial": med / ndm,
              "channel_samples_per_s": ndm * nout * nchans / (med * 1e-3),
              "algorithmic_bytes_per_s": (nsamp * nchans + ndm * nout * 4) / (med * 1e-3),
              "search_ms_per_trial_bench_r06_cfg2": search_ms,
              "dedisperse_to_search_ratio": (med / ndm) / search_ms,
              "source_digest": bench.source_digest(), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
