"""The pass-0 launches in leaf-span order (plan.cpp order_launch_units) on the
device: a plan with several rungs and many pass-0 units per transform at
batch 3 (the trial loop, an odd batch), with 21 transforms per rung and with
bins 255-258, which straddle the 4/5-slot boundary so both launches reorder.
Every trial against the strict oracle and bit-identical to its batch-1 run."""
import numpy as np
import pytest

import inputs
from conftest import snr_close

pytestmark = pytest.mark.gpu

N, TSAMP, PMIN, PMAX = 1 << 18, 256e-6, 0.1, 1.0


@pytest.mark.parametrize("bmin,bmax", [(240, 260), (255, 258)])
def test_reordered_pass0_matches_oracle(oracle, bmin, bmax):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from riptide_amd import engine
    its = engine.schedule_items(N, TSAMP, PMIN, PMAX, bmin, bmax)
    p0 = its[its["pass"] == 0]
    assert len({(int(l), int(s)) for l, s in zip(p0["launch"], p0["slots"])}) >= 2       # 4- and 5-slot launches
    for l in np.unique(p0["launch"]):
        L = p0[p0["launch"] == l]
        assert np.unique(L["xform"]).size > np.unique(L["rung"]).size                    # the launch reorders
    plan = engine.PeriodogramPlan.for_search(N, TSAMP, PMIN, PMAX, bmin, bmax, ducy_max=0.05)
    xs = np.stack([inputs.with_signal(N, TSAMP, 70 + s, 0.23 + 0.17 * s, 11.0) for s in range(3)])
    d = torch.from_numpy(xs).cuda()
    batch = plan.run(d, check=True).cpu().numpy()
    periods, foldbins = plan.grid()
    widths = np.asarray(plan.widths, dtype=np.uint64)
    for b in range(3):
        single = plan.run(d[b:b + 1].contiguous(), check=True).cpu().numpy()[0]
        assert np.array_equal(batch[b], single), f"trial {b} differs from its batch-1 run"
        op, ofb, osnr = oracle.periodogram(xs[b], TSAMP, widths, PMIN, PMAX, bmin, bmax)
        assert np.array_equal(periods, op) and np.array_equal(foldbins, ofb)
        ok, msg = snr_close(batch[b], osnr, rtol=2e-6)
        assert ok, f"trial {b}: {msg}"
