"""Time the candidate refinement (rt_refine_device through
engine.refine_device) on device-resident buffers: by default 64 candidates of
32 bands x 32 sub-integrations x 256 bins over a grid of 65 DM x 33 period
trials at the default widths, Gaussian cubes and random shift tables.  Between
two HIP events per call (both stages; the output and workspace allocations of
engine.refine_device come from torch's caching allocator, warm after the first
call); two warm-ups, then the median of --repeats calls.

Three yardsticks beside it:
  host_spec   rt_refine_host on one core, timed on --host-cands candidates and
              scaled to the job
  numpy       the numpy restatement (roll and add, then the boxcar S/N from a
              prefix sum), timed on one candidate and scaled
  alg_bytes   the call's algorithmic bytes -- the cube read once per DM trial,
              y written and read, the S/N written -- divided by the time
A record, not a gate: prints one JSON line and writes it to --out.

    python tools/bench_refine.py --out profiles/refine_64x32x32x256.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def numpy_refine(x, dshift, pshift, widths, stdnoise):
    """The restatement a user would write on the host: snr [K, J, W]."""
    B, S, N = x.shape
    K, J = dshift.shape[0], pshift.shape[0]
    n = np.arange(N)
    out = np.empty((K, J, len(widths)), dtype=np.float32)
    for k in range(K):
        y = np.zeros((S, N), dtype=np.float32)
        for b in range(B):
            y += np.roll(x[b], -int(dshift[k, b]), axis=1)
        for j in range(J):
            idx = (n[None, :] + pshift[j][:, None]) % N
            p = np.take_along_axis(y, idx, axis=1).sum(axis=0, dtype=np.float32)
            cps = np.cumsum(np.concatenate([p, p]), dtype=np.float64).astype(np.float32)
            total = cps[N - 1]
            for iw, w in enumerate(widths):
                w = int(w)
                h = np.sqrt((N - w) / float(N * w))
                b_ = w / float(N - w) * h
                dmax = (cps[w:w + N] - cps[:N]).max()
                out[k, j, iw] = ((h + b_) * dmax - b_ * total) / stdnoise
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--bands", type=int, default=32)
    ap.add_argument("--subints", type=int, default=32)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--ndm", type=int, default=65)
    ap.add_argument("--nper", type=int, default=33)
    ap.add_argument("--host-cands", type=int, default=2)
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")
    import torch
    from riptide_amd import engine, generate_width_trials
    from riptide_amd.refine import pack_refine, refine_host
    C, B, S, N, K, J = args.cands, args.bands, args.subints, args.bins, args.ndm, args.nper
    widths = generate_width_trials(N).astype(np.uint32)
    W = widths.size
    stdnoise = float(np.sqrt(B))
    rng = np.random.RandomState(0)
    jobs = [(rng.normal(size=(B, S, N)).astype(np.float32), rng.randint(0, N, size=(K, B)).astype(np.int32),
             rng.randint(0, N, size=(J, S)).astype(np.int32), widths, stdnoise) for _ in range(C)]
    cubes, shifts, wd, table, _, nsnr, _ = pack_refine(jobs)
    dev = torch.device("cuda", 0)
    d_cubes = torch.from_numpy(cubes).to(dev)
    d_shifts = torch.from_numpy(shifts).to(dev)
    d_widths = torch.from_numpy(wd.astype(np.int32)).to(dev)

    def call():
        return engine.refine_device(d_cubes, d_shifts, d_widths, table)[0]
    for _ in range(2):
        snr = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        snr = call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    dev_snr = snr.cpu().numpy()

    # one-core specification and the numpy restatement, on a few candidates
    hc = max(1, min(args.host_cands, C))
    t0 = time.perf_counter()
    host = [refine_host(*jobs[i]) for i in range(hc)]
    host_ms = (time.perf_counter() - t0) * 1e3 / hc * C
    t0 = time.perf_counter()
    ref = numpy_refine(*jobs[0])
    numpy_ms = (time.perf_counter() - t0) * 1e3 * C
    per = K * J * W
    err_host = max(float(np.abs(dev_snr[i * per:(i + 1) * per].reshape(K, J, W) - host[i]).max()) for i in range(hc))
    err_numpy = float(np.abs(host[0] - ref).max())

    alg_bytes = C * 4.0 * (K * B * S * N + 2 * K * S * N + K * J * W)
    result = {
        "kind": "refine", "cands": C, "bands": B, "subints": S, "bins": N, "ndm": K, "nper": J, "widths": W,
        "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
        "device_ms": ms, "device_ms_min": float(min(times)), "device_ms_max": float(max(times)),
        "us_per_candidate": ms * 1e3 / C,
        "host_spec_ms_one_core": host_ms, "host_cands_timed": hc, "numpy_ms": numpy_ms,
        "speedup_vs_host_spec": host_ms / ms, "speedup_vs_numpy": numpy_ms / ms,
        "alg_bytes": alg_bytes, "alg_GBps": alg_bytes / (ms * 1e-3) / 1e9,
        # shifted adds of both stages, and what they read: LDS bytes when the slices are staged
        "adds": float(C) * (K * B * S * N + K * J * S * N),
        "lds_read_GBps": float(C) * 4.0 * (K * B * S * N + K * J * S * N) / (ms * 1e-3) / 1e9,
        "max_abs_snr_diff_device_vs_host_spec": err_host, "max_abs_snr_diff_host_spec_vs_numpy": err_numpy,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
