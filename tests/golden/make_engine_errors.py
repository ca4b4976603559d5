"""The error table of the device wrappers of riptide_amd.engine for bad
arguments that are refused on the host, before any device call.  Writes
tests/golden/engine_errors.json: a list of [case name, exception type,
message].  tests/test_engine_args_host.py replays cases() and asserts the table
entry for entry, so the table is recorded before the wrappers' argument checks
are touched, never from the code under test.  No GPU is needed.

Every wrapper refuses a tensor that is not on a device first, so each bad
argument below is a host tensor: the wrong dtype, a 3-D tensor, a non-unit
stride and a non-contiguous block are all met on host tensors, and the table
pins that they are refused, with which message, and that the block is judged
before a mask or an `out`.

Not in the table, because the call gets as far as a device call here (asking
for the current stream or allocating) -- tests/test_gpu_engine_args.py has
them:
  - a mask of the wrong length on a device block (a host block is refused
    first: the "mask of the wrong length" cases below pin that order);
  - a workspace or an `out` of the wrong size, dtype or device;
  - overlapping rows (stride(0) < N) of single_pulse_device / resample_device.
PeriodogramPlan cannot be built without a device (the constructor uploads the
plan).  run / ladder / passes check their tensors against the plan's device
and size before they use the plan's handle, so they are called here on a plan
object whose constructor did not run, with those attributes set by hand.

Usage:  python tests/golden/make_engine_errors.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "engine_errors.json")


def _unbuilt_plan(engine, torch):
    plan = object.__new__(engine.PeriodogramPlan)
    plan.device, plan.size, plan.length, plan.num_widths = torch.device("cuda", 0), 64, 5, 3
    return plan


def cases():
    """[(case name, thunk)]: every thunk raises on the host."""
    import torch
    from riptide_amd import engine
    f32 = torch.zeros((2, 64), dtype=torch.float32)
    bad_rows = {
        "cpu tensor": f32,
        "cpu 1-D tensor": f32[0],
        "wrong dtype": f32.double(),
        "3-D tensor": f32.reshape(2, 8, 8),
        "non-unit stride": torch.zeros((2, 128), dtype=torch.float32)[:, ::2],
    }
    rows = {
        "deredden_normalise": lambda x: engine.deredden_normalise(x, 9, 3),
        "deredden_normalise with out and workspace":
            lambda x: engine.deredden_normalise(x, 9, 3, out=torch.zeros(1), workspace=torch.zeros(1)),
        "fold_device": lambda x: engine.fold_device(x, 1e-3, [(0, 0.016, 16, None)]),
        "fold_device without specs": lambda x: engine.fold_device(x, 1e-3, []),
        "single_pulse_device": lambda x: engine.single_pulse_device(x, [1, 2], 8.0),
        "single_pulse_device without widths": lambda x: engine.single_pulse_device(x, [], 8.0),
        "resample_device": lambda x: engine.resample_device(x, [0.0]),
        "resample_device with out": lambda x: engine.resample_device(x, [0.0], out=torch.zeros(1)),
    }
    out = [(f"{name}: {bad}", lambda fn=fn, x=x: fn(x)) for name, fn in rows.items() for bad, x in bad_rows.items()]

    u8 = torch.zeros((32, 8), dtype=torch.uint8)
    bad_blocks = {
        "cpu tensor": u8,
        "wrong dtype": u8.double(),
        "3-D tensor": u8.reshape(32, 4, 2),
        "non-contiguous block": torch.zeros((32, 16), dtype=torch.uint8)[:, ::2],
        "1-D tensor": u8[0],
    }
    delays = torch.zeros((2, 8), dtype=torch.int32)
    bands = np.array([[0, 4], [4, 8]], dtype=np.uint32)
    short_mask = torch.zeros(7, dtype=torch.uint8)
    cell_mask = engine.DeviceBlockMask(torch.zeros((4, 8), dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8), 8)
    blocks = {
        "zero_dm_mean_device": lambda b: engine.zero_dm_mean_device(b),
        "zero_dm_mean_device, mask of the wrong length": lambda b: engine.zero_dm_mean_device(b, mask=short_mask),
        "zero_dm_mean_device with out and block mask":
            lambda b: engine.zero_dm_mean_device(b, out=torch.zeros(1), block_mask=cell_mask),
        "zero_dm_mean_device packed": lambda b: engine.zero_dm_mean_device(b, nbits=3),
        "block_stats_device": lambda b: engine.block_stats_device(b, 8),
        "block_stats_device, block_len 0": lambda b: engine.block_stats_device(b, 0),
        "block_stats_device with out and workspace":
            lambda b: engine.block_stats_device(b, 8, out=torch.zeros(1), workspace=torch.zeros(1)),
        "channel_stats_device": lambda b: engine.channel_stats_device(b, torch.zeros((2, 8), dtype=torch.float64)),
        "channel_stats_device, acc of the wrong shape":
            lambda b: engine.channel_stats_device(b, torch.zeros(3), workspace=torch.zeros(1)),
        "dedisperse_device": lambda b: engine.dedisperse_device(b, delays, 4),
        "dedisperse_device, mask of the wrong length":
            lambda b: engine.dedisperse_device(b, delays, 4, mask=short_mask),
        "dedisperse_device, max_delay beyond the block": lambda b: engine.dedisperse_device(b, delays, 99),
        "dedisperse_device with out, workspace and block mask":
            lambda b: engine.dedisperse_device(b, delays, 4, out=torch.zeros(1), workspace=torch.zeros(1),
                                               block_mask=cell_mask),
        "dedisperse_bands_device": lambda b: engine.dedisperse_bands_device(b, delays, 4, bands),
        "dedisperse_bands_device, mask of the wrong length":
            lambda b: engine.dedisperse_bands_device(b, delays, 4, bands, mask=short_mask),
        "dedisperse_bands_device, bands of the wrong shape":
            lambda b: engine.dedisperse_bands_device(b, delays, 4, bands.ravel()),
    }
    out += [(f"{name}: {bad}", lambda fn=fn, b=b: fn(b)) for name, fn in blocks.items()
            for bad, b in bad_blocks.items()]

    flat = torch.zeros(16, dtype=torch.float32)
    i32 = torch.zeros(16, dtype=torch.int32)
    bad_flat = {
        "cpu cubes": (flat, i32, i32),
        "cubes of the wrong dtype": (flat.double(), i32, i32),
        "2-D cubes": (flat.reshape(4, 4), i32, i32),
        "strided cubes": (torch.zeros(32, dtype=torch.float32)[::2], i32, i32),
    }
    out += [(f"refine_device: {bad}", lambda a=a: engine.refine_device(*a, np.zeros(0, dtype=np.uint8)))
            for bad, a in bad_flat.items()]

    plan = _unbuilt_plan(engine, torch)
    ws = torch.zeros(16, dtype=torch.uint8)
    bad_series = dict(bad_rows, **{"wrong length": torch.zeros((2, 65), dtype=torch.float32)})
    for bad, x in bad_series.items():
        out.append((f"PeriodogramPlan.run: {bad}", lambda x=x: plan.run(x)))
        out.append((f"PeriodogramPlan.run with out, workspace: {bad}", lambda x=x: plan.run(x, out=ws, workspace=ws)))
        if x.dim() > 1:     # ladder takes [B, size] alone
            out.append((f"PeriodogramPlan.ladder: {bad}", lambda x=x: plan.ladder(x, ws)))
    bad_out = {
        "cpu tensor": torch.zeros((2, 5, 3), dtype=torch.float32),
        "wrong dtype": torch.zeros((2, 5, 3), dtype=torch.float64),
        "wrong shape": torch.zeros((2, 5, 4), dtype=torch.float32),
        "2-D tensor": torch.zeros((2, 15), dtype=torch.float32),
    }
    out += [(f"PeriodogramPlan.passes: {bad}", lambda o=o: plan.passes(o, ws)) for bad, o in bad_out.items()]
    return out


def outcome(thunk):
    """[exception type, message] of a thunk, or None when it did not raise."""
    try:
        thunk()
    except Exception as e:      # noqa: BLE001  (the type is what is recorded)
        return [type(e).__name__, str(e)]
    return None


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    table, dropped = [], []
    for name, thunk in cases():
        got = outcome(thunk)
        # a wrapper that got as far as a device call fails here with torch's or the runtime's own error
        (table if got is not None and got[0] == "ValueError" else dropped).append([name] + (got or ["-", "no error"]))
    with open(OUT, "w") as f:
        json.dump(table, f, indent=0)
        f.write("\n")
    print(f"{len(table)} cases -> {OUT}")
    for row in dropped:
        print("dropped (not a host-side ValueError):", row)


if __name__ == "__main__":
    main()
