"""Time a DM plan against the native-resolution search of the same DMs on the
d01a shape: 1024 channels x 2^22 uint8 samples of a 1.2-1.5 GHz band at
256 us, written to a file in --dir (page cache warm) and streamed.

  plan     dedispersion.dm_plan(freqs, tsamp, dm_max=1000): timed are
           dedisperse_filterbank_plan and search_filterbank_plan
  native   the plan's flat DM list through dedisperse_filterbank and
           search_filterbank, which this change leaves as they were, in slices
           that fit the budget
  f1       a plan of the same DMs all at f = 1 against dedisperse_filterbank:
           the step-table path with nothing to decimate
  ladder   the same DMs in four equal parts at f = 1, 2, 4, 8
           (DMPlan.from_steps): each part's search alone, so a step's cost can
           be set against 1 / f of the f = 1 part's

Host clock around each call, ended by a device synchronise; one warm-up per
shape, then --repeats calls, plan and native alternating; medians with min and
max, which are the run-to-run spread.  The plan's f = 1 rows must equal the
native rows bit for bit.  A record, not a gate: prints one JSON line and
writes it to --out.

    python tools/bench_dm_plan.py --out profiles/dp01a_dm_plan.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DEREDDEN = {"rmed_width": 5.0, "rmed_minpts": 101}
RANGES = [{"name": "bench", "ffa_search": {"period_min": 1.0, "period_max": 10.0, "bins_min": 240, "bins_max": 260},
           "find_peaks": {"smin": 7.0}}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nchans", type=int, default=1024)
    ap.add_argument("--log2-nsamp", type=int, default=22)
    ap.add_argument("--dm-max", type=float, default=1000.0)
    ap.add_argument("--slice", type=int, default=1024, help="DMs per native call: as many as fit the budget")
    ap.add_argument("--dir", default="/tmp")
    args = ap.parse_args()
    import torch
    import bench
    from riptide_amd.dedispersion import DMPlan, dedisperse_filterbank, dedisperse_filterbank_plan, dm_plan
    from riptide_amd.dispatch import EngineSearcher
    from riptide_amd.reading import open_filterbank, write_sigproc

    nchans, nsamp, tsamp = args.nchans, 1 << args.log2_nsamp, 256e-6
    freqs = 1500.0 - (300.0 / nchans) * np.arange(nchans)
    plan = dm_plan(freqs, tsamp, dm_max=args.dm_max)
    dms = plan.dms
    torch.cuda.set_device(0)
    fname = os.path.join(args.dir, "bench_dm_plan.fil")
    rng = np.random.RandomState(0)
    tile = rng.randint(0, 256, size=(4096, nchans)).astype(np.uint8)
    write_sigproc(fname, np.tile(tile, (nsamp // 4096, 1)),
                  {"tsamp": tsamp, "nbits": 8, "fch1": float(freqs[0]), "foff": float(freqs[1] - freqs[0]),
                   "nchans": nchans, "nifs": 1})
    fb = open_filterbank(fname)
    searcher = EngineSearcher(DEREDDEN, RANGES, device=0, batch=8)
    slices = [list(dms[i:i + args.slice]) for i in range(0, dms.size, args.slice)]
    L = dedisperse_filterbank_plan(fb, DMPlan.from_steps([(dms[-1:], 1)]))[0].shape[1]    # the plan's native length

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def native_dedisperse():
        for part in slices:
            dedisperse_filterbank(fb, part, nout=L)

    def native_search():
        for part in slices:
            searcher.search_filterbank(fb, part, nout=L)

    def alternating(fns):
        """{name: [ms]}: one warm-up of each, then --repeats rounds, one call of each in turn."""
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(args.repeats):
            for name, fn in fns.items():
                ms[name].append(clock(fn))
        return ms

    def summary(ms):
        return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}

    # results must not change: the plan's f = 1 rows are the native rows
    first = plan.steps[0]
    if first.downsamp == 1:
        got = dedisperse_filterbank_plan(fb, plan)[0]
        ref = dedisperse_filterbank(fb, list(first.dms[:args.slice]), nout=L)
        assert torch.equal(got[:ref.shape[0]], ref), "the plan's f = 1 step differs from dedisperse_filterbank"
        del got, ref
    f1 = DMPlan.from_steps([(dms, 1)], tsamp)
    quarters = np.array_split(dms, 4)
    ladder = DMPlan.from_steps([(q, f) for q, f in zip(quarters, (1, 2, 4, 8))], tsamp)
    ded = alternating({"plan": lambda: dedisperse_filterbank_plan(fb, plan), "native": native_dedisperse,
                       "f1": lambda: dedisperse_filterbank_plan(fb, f1)})
    srch = alternating({"plan": lambda: searcher.search_filterbank_plan(fb, plan), "native": native_search,
                        "ladder": lambda: searcher.search_filterbank_plan(fb, ladder)})

    def per_step(p):
        rows = []
        for s in p.steps:
            one = DMPlan([(s.dms, s.downsamp)], tsamp, p.dm_cover)
            ms = alternating({"d": lambda: dedisperse_filterbank_plan(fb, one),
                              "s": lambda: searcher.search_filterbank_plan(fb, one)})
            rows.append({"downsamp": s.downsamp, "ndm": int(s.dms.size), "dm_first": float(s.dms[0]),
                         "dm_last": float(s.dms[-1]), "dedisperse": summary(ms["d"]), "search": summary(ms["s"]),
                         "search_ms_per_dm": float(np.median(ms["s"])) / s.dms.size})
        return rows

    plan_steps, ladder_steps = per_step(plan), per_step(ladder)
    os.remove(fname)
    base = ladder_steps[0]["search_ms_per_dm"]
    for row in ladder_steps:
        row["search_per_dm_over_f1"] = row["search_ms_per_dm"] / base
        row["expected_one_over_f"] = 1.0 / row["downsamp"]
    result = {"nchans": nchans, "nsamp": nsamp, "tsamp": tsamp, "dm_max": args.dm_max, "ndm": int(dms.size),
              "plan": repr(plan), "plan_factors": sorted({int(f) for f in plan.downsamp}), "native_nout": int(L),
              "repeats": args.repeats, "native_slice": args.slice,
              "dedisperse_plan": summary(ded["plan"]), "dedisperse_native": summary(ded["native"]),
              "dedisperse_f1_plan": summary(ded["f1"]),
              "dedisperse_plan_to_native_ratio": float(np.median(ded["plan"]) / np.median(ded["native"])),
              "dedisperse_f1_plan_to_native_ratio": float(np.median(ded["f1"]) / np.median(ded["native"])),
              "search_plan": summary(srch["plan"]), "search_native": summary(srch["native"]),
              "search_ladder": summary(srch["ladder"]),
              "search_plan_to_native_ratio": float(np.median(srch["plan"]) / np.median(srch["native"])),
              "search_ladder_to_native_ratio": float(np.median(srch["ladder"]) / np.median(srch["native"])),
              "plan_steps": plan_steps, "ladder_steps": ladder_steps,
              "source_digest": bench.source_digest(), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
