"""Device-side argument cases of the engine wrappers: what a host tensor cannot
reach (tests/test_engine_args_host.py has the rest).  A workspace one byte
short, of the wrong dtype or on the host, an `out` of the wrong shape, a mask
of the wrong length and overlapping rows are refused with the messages the
wrappers had before their checks were shared -- the strings below are copied
from that source -- and nothing is launched.  The one call that launches: the
dereddening of a [2, 64] slice of a [2, 80] tensor, read in place."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, N = 2, 64                      # rows
NSAMP, NCHANS, BLOCK_LEN = 32, 8, 8
MAX_DELAY = 4
WS, MINPTS = 9, 3                 # dereddening window and its least points, for 64 samples
NOUT = NSAMP - MAX_DELAY


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    return torch


@pytest.fixture(scope="module")
def engine(torch):
    from riptide_amd import engine
    return engine


@pytest.fixture(scope="module")
def args(torch, engine):
    """The good arguments, made once: nothing below writes to them."""
    dev = torch.device("cuda", torch.cuda.current_device())
    plan = engine.PeriodogramPlan.for_search(4096, 1e-3, 0.3, 1.0, 240, 260)
    return {
        "dev": dev,
        "rows": torch.zeros((B, N), dtype=torch.float32, device=dev),
        "block": torch.zeros((NSAMP, NCHANS), dtype=torch.uint8, device=dev),
        "delays": torch.zeros((2, NCHANS), dtype=torch.int32, device=dev),
        "bands": np.array([[0, 4], [4, 8], [0, 8]], dtype=np.uint32),
        "acc": torch.zeros((2, NCHANS), dtype=torch.float64, device=dev),
        "plan": plan,
        "series": torch.zeros((B, plan.size), dtype=torch.float32, device=dev),
        "snr": torch.empty((B, plan.length, plan.num_widths), dtype=torch.float32, device=dev),
        # block_len 8 needs no workspace (none up to 2048): the short workspace is tried on longer blocks
        "long_block": torch.zeros((4100, NCHANS), dtype=torch.uint8, device=dev),
    }


def workspace_calls(engine, a):
    """{name: (call taking a workspace, bytes it needs, whose device the message names)}"""
    plan = a["plan"]
    return {
        "run": (lambda ws: plan.run(a["series"], workspace=ws), plan.workspace_bytes(B), "plan"),
        "ladder": (lambda ws: plan.ladder(a["series"], ws), plan.workspace_bytes(B), "plan"),
        "passes": (lambda ws: plan.passes(a["snr"], ws), plan.workspace_bytes(B), "plan"),
        "deredden_normalise": (lambda ws: engine.deredden_normalise(a["rows"], WS, MINPTS, workspace=ws),
                               engine.deredden_workspace_bytes(N, WS, MINPTS, B), "data"),
        "block_stats_device": (lambda ws: engine.block_stats_device(a["block"], BLOCK_LEN, workspace=ws),
                               engine.block_stats_workspace_bytes(NSAMP, NCHANS, BLOCK_LEN), "block"),
        "block_stats_device, long blocks": (lambda ws: engine.block_stats_device(a["long_block"], 4096, workspace=ws),
                                            engine.block_stats_workspace_bytes(4100, NCHANS, 4096), "block"),
        "channel_stats_device": (lambda ws: engine.channel_stats_device(a["block"], a["acc"], workspace=ws),
                                 engine.channel_stats_workspace_bytes(NSAMP, NCHANS), "block"),
        "dedisperse_device": (lambda ws: engine.dedisperse_device(a["block"], a["delays"], MAX_DELAY, workspace=ws),
                              engine.dedisperse_workspace_bytes("uint8", NSAMP, NCHANS), "block"),
        "dedisperse_device, zero_dm":
            (lambda ws: engine.dedisperse_device(a["block"], a["delays"], MAX_DELAY, workspace=ws, zero_dm=True),
             engine.dedisperse_workspace_bytes("uint8", NSAMP, NCHANS, zero_dm=True), "block"),
        "dedisperse_bands_device":
            (lambda ws: engine.dedisperse_bands_device(a["block"], a["delays"], MAX_DELAY, a["bands"], workspace=ws),
             engine.dedisperse_workspace_bytes("uint8", NSAMP, NCHANS), "block"),
    }


WORKSPACE_CALLS = ("run", "ladder", "passes", "deredden_normalise", "block_stats_device",
                   "block_stats_device, long blocks", "channel_stats_device", "dedisperse_device",
                   "dedisperse_device, zero_dm", "dedisperse_bands_device")


@pytest.mark.parametrize("name", WORKSPACE_CALLS)
def test_bad_workspace_is_refused(torch, engine, args, name):
    calls = workspace_calls(engine, args)
    assert tuple(calls) == WORKSPACE_CALLS
    call, need, whose = calls[name]
    message = f"workspace must be a contiguous uint8 tensor of >= {need} bytes on the {whose}'s device"
    bad = {
        "wrong dtype": torch.empty(need + 16, dtype=torch.int8, device=args["dev"]),
        "on the host": torch.empty(need + 16, dtype=torch.uint8),
        "not contiguous": torch.empty(2 * need + 32, dtype=torch.uint8, device=args["dev"])[::2],
    }
    if name == "block_stats_device":
        assert need == 0                # no workspace can be too short for it
    else:
        assert need > 0
        bad["one byte short"] = torch.empty(need - 1, dtype=torch.uint8, device=args["dev"])
    for what, ws in bad.items():
        with pytest.raises(ValueError) as e:
            call(ws)
        assert str(e.value) == message, what
    if name in ("ladder", "passes"):    # these two do not allocate one
        with pytest.raises(ValueError) as e:
            call(None)
        assert str(e.value) == message


def test_out_of_the_wrong_shape_is_refused(torch, engine, args):
    a, plan, dev = args, args["plan"], args["dev"]
    L, W = plan.length, plan.num_widths

    def f32(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)

    calls = [
        (lambda: plan.run(a["series"], out=f32(B, L, W + 1)),
         f"out must be a contiguous float32 [{B}, {L}, {W}] tensor on the plan's device"),
        (lambda: plan.run(a["series"], out=f32(B, L, 2 * W)[:, :, ::2]),
         f"out must be a contiguous float32 [{B}, {L}, {W}] tensor on the plan's device"),
        (lambda: plan.passes(f32(B, L, W + 1), torch.empty(plan.workspace_bytes(B), dtype=torch.uint8, device=dev)),
         f"out must be a contiguous float32 [B, {L}, {W}] tensor on the plan's device"),
        (lambda: engine.deredden_normalise(a["rows"], WS, MINPTS, out=f32(B, N + 1)),
         "out must be float32 [B, N] rows with unit stride on the data's device"),
        (lambda: engine.deredden_normalise(a["rows"], WS, MINPTS, out=f32(B, 2 * N)[:, ::2]),
         "out must be float32 [B, N] rows with unit stride on the data's device"),
        (lambda: engine.resample_device(a["rows"], [0.0], out=f32(B, N + 1)),
         f"out must be float32 [{B}, {N}] rows with unit stride on the data's device"),
        (lambda: engine.resample_device(a["rows"], [0.0], out=f32(B * N).as_strided((B, N), (N // 2, 1))),
         "resample: output row stride below the series length"),
        (lambda: engine.zero_dm_mean_device(a["block"], out=f32(NSAMP + 1)),
         f"out must be a contiguous float32 [{NSAMP}] tensor on the block's device"),
        (lambda: engine.block_stats_device(a["block"], BLOCK_LEN,
                                           out=torch.empty((4, 1, NCHANS), dtype=torch.float64, device=dev)),
         f"out must be a contiguous float64 [4, 2, {NCHANS}] tensor on the block's device"),
        (lambda: engine.block_stats_device(a["block"], BLOCK_LEN, out=f32(4, 2, NCHANS)),
         f"out must be a contiguous float64 [4, 2, {NCHANS}] tensor on the block's device"),
        (lambda: engine.dedisperse_device(a["block"], a["delays"], MAX_DELAY, out=f32(2, NOUT - 1)),
         f"out must be float32 [2, >= {NOUT}] rows with unit stride on the block's device"),
        (lambda: engine.dedisperse_device(a["block"], a["delays"], MAX_DELAY, out=f32(2, NOUT + 2), out_offset=3),
         f"out must be float32 [2, >= {NOUT + 3}] rows with unit stride on the block's device"),
        (lambda: engine.dedisperse_device(a["block"], a["delays"], MAX_DELAY, out=f32(3, NOUT)),
         f"out must be float32 [2, >= {NOUT}] rows with unit stride on the block's device"),
        (lambda: engine.dedisperse_bands_device(a["block"], a["delays"], MAX_DELAY, a["bands"], out=f32(2, 2, NOUT)),
         f"out must be a contiguous float32 [2, 3, >= {NOUT}] tensor on the block's device"),
        (lambda: engine.dedisperse_bands_device(a["block"], a["delays"], MAX_DELAY, a["bands"],
                                                out=f32(2, 3, NOUT - 1)),
         f"out must be a contiguous float32 [2, 3, >= {NOUT}] tensor on the block's device"),
    ]
    for k, (call, message) in enumerate(calls):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message, k


def test_masks_and_overlapping_rows_are_refused(torch, engine, args):
    a = args
    short = torch.zeros(NCHANS - 1, dtype=torch.uint8, device=a["dev"])
    overlapping = torch.zeros(B * N, dtype=torch.float32, device=a["dev"]).as_strided((B, N), (N // 2, 1))
    calls = [
        (lambda: engine.zero_dm_mean_device(a["block"], mask=short),
         "mask must be a contiguous uint8 [nchans] tensor on the block's device"),
        (lambda: engine.dedisperse_device(a["block"], a["delays"], MAX_DELAY, mask=short),
         "mask must be a contiguous uint8 [nchans] tensor on the block's device"),
        (lambda: engine.dedisperse_bands_device(a["block"], a["delays"], MAX_DELAY, a["bands"], mask=short.cpu()),
         "mask must be a contiguous uint8 [nchans] tensor on the block's device"),
        (lambda: engine.single_pulse_device(overlapping, [1, 2], 8.0), "data rows must not overlap"),
        (lambda: engine.resample_device(overlapping, [0.0]), "resample: input row stride below the series length"),
        (lambda: engine.channel_stats_device(a["block"], a["acc"][:, :-1]),
         f"acc must be a contiguous float64 [2, {NCHANS}] tensor on the block's device"),
    ]
    for k, (call, message) in enumerate(calls):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message, k


def test_deredden_normalise_reads_a_slice_in_place(torch, engine, args):
    """A [2, 64] slice of a [2, 80] tensor is accepted and gives the bits of
    its contiguous copy, into a strided `out` as well."""
    wide = torch.from_numpy(np.random.RandomState(5).normal(size=(B, 80)).astype(np.float32)).to(args["dev"])
    x = wide[:, :N]
    assert x.stride(0) == 80 and not x.is_contiguous()
    ref = engine.deredden_normalise(x.contiguous(), WS, MINPTS)
    got = engine.deredden_normalise(x, WS, MINPTS)
    assert got.is_contiguous() and torch.equal(got.view(torch.int32), ref.view(torch.int32))
    into = torch.full((B, 80), float("nan"), dtype=torch.float32, device=args["dev"])
    assert engine.deredden_normalise(x, WS, MINPTS, out=into[:, :N]).data_ptr() == into.data_ptr()
    assert torch.equal(into[:, :N].view(torch.int32), ref.view(torch.int32)) and bool(torch.isnan(into[:, N:]).all())
    assert torch.equal(engine.deredden_normalise(x[0], WS, MINPTS).view(torch.int32), ref[0].view(torch.int32))
