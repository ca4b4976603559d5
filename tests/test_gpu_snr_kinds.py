"""Final cone launches by S/N kind on the device: plans whose final units run
in both the segmented instance (240-264 bins, widths <= 9) and the row-group
instance of the 4-slot and the 5-slot bucket, with a trial-loop tail in each
(batch 3 at two trials per workgroup), and a unit of the wrong kind for its
launch's instance (test build of the library)."""
import os
import sys

import numpy as np
import pytest

import inputs
from conftest import snr_close

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 6, 9]
N = 1 << 17
# astride 239 | 240 (4-slot bucket), 264 | 265 (5-slot), and a range all in the
# 5-slot bucket (257-320 bins) astride 264 | 265
RANGES = [(238, 242), (262, 266), (257, 266)]


@pytest.mark.parametrize("bmin,bmax", RANGES, ids=[f"{a}-{b}" for a, b in RANGES])
def test_final_kinds_trial_loop(oracle, monkeypatch, bmin, bmax):
    """One plan with segmented and row-group final launches, a batch of three
    distinct trials at RIPTIDE_AMD_TRIALS_PER_WG=2 (workgroups of two trials
    and a tail of one): trial 0 within 2e-6 of max(|S/N|, 1) of the strict C
    oracle (the project's bound for the fused S/N: the same additions per
    step), trials 1 and 2 bit-identical to their own batch-1 runs, and the
    whole batch bit-identical to the plan built and run with the kConeSnrSeg
    feature bit off (every final unit row-group)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from riptide_amd import engine
    tsamp = inputs.SNR_SHAPE_TSAMP
    c = inputs.snr_shape_plan(bmin, bmax, N)
    w = np.asarray(WIDTHS, dtype=np.uint64)
    xs = np.stack([inputs.with_signal(N, tsamp, 7 * bmin + s, (bmin + (0.3 + 0.2 * s) * (bmax - bmin)) * tsamp * 1.003, 8.0)
                   for s in range(3)])
    operiods, ofoldbins, osnr = oracle.periodogram(xs[0], tsamp, w, c["pmin"], c["pmax"], bmin, bmax)
    assert np.isfinite(osnr).all()
    monkeypatch.setenv("RIPTIDE_AMD_TRIALS_PER_WG", "2")
    args = (c["pmin"], c["pmax"], bmin, bmax)
    plan = engine.PeriodogramPlan(N, tsamp, w, *args)
    st = plan.stats()
    assert st["items"] > st["transforms"]            # tile finals
    periods, foldbins = plan.grid()
    assert np.array_equal(periods, operiods) and np.array_equal(foldbins, ofoldbins)
    assert set(range(bmin, bmax + 1)) <= set(foldbins.tolist())
    d = torch.from_numpy(xs).cuda()
    batch = plan.run(d, check=True).cpu().numpy()
    err = float((np.abs(batch[0].astype(np.float64) - osnr) / np.maximum(np.abs(osnr), 1.0)).max())
    print(f"final kinds bins {bmin}-{bmax}: L={periods.size} scaled err vs oracle {err:.3e}")
    ok, msg = snr_close(batch[0], osnr, rtol=2e-6)
    assert ok, msg
    for b in (1, 2):
        single = plan.run(d[b:b + 1].contiguous(), check=True).cpu().numpy()[0]
        assert np.array_equal(batch[b], single), f"trial {b} of the batch differs from its batch-1 run"
    monkeypatch.setenv("RIPTIDE_AMD_CONE_FLAGS", "7")
    try:
        wplan = engine.PeriodogramPlan(N, tsamp, w, *args)
        wbatch = wplan.run(d, check=True).cpu().numpy()
    finally:
        monkeypatch.delenv("RIPTIDE_AMD_CONE_FLAGS")
    assert wplan.stats()["moved_bytes"] != st["moved_bytes"], "no segmented final tiles"
    assert np.array_equal(batch, wbatch), "segmented launches differ from the all-row-group plan"


_MISKIND_BODY = r"""
import sys
import numpy as np
import pytest
import torch
sys.path[:0] = [REPO, GOLDEN]
import inputs
from riptide_amd import _lib, engine
assert _lib.LIB_PATH.endswith("libriptide_amd_testhooks.so")
c = inputs.snr_shape_plan(238, 242, 1 << 17)
w = np.asarray([1, 2, 3, 4, 6, 9], dtype=np.uint64)
x = torch.from_numpy(inputs.with_signal(c["n"], c["tsamp"], 5, 0.2401, 8.0)).cuda()
args = (c["n"], c["tsamp"], w, c["pmin"], c["pmax"], 238, 242)
good = engine.PeriodogramPlan(*args)
good.run(x, check=True)
lib = _lib.load()
lib.rt_test_corrupt_next_plans(2)      # the first segmented unit marked row-group
try:
    bad = engine.PeriodogramPlan(*args)
    with pytest.raises(_lib.EngineError):
        bad.run(x, check=True)
    bad.check()                        # the flag was cleared by the failed check
finally:
    lib.rt_test_corrupt_next_plans(0)
good.check()
print("mis-kinded unit OK")
"""


def test_miskinded_unit_raises():
    """A unit whose S/N kind disagrees with its launch's kernel instance (a
    row-group unit in a segmented launch) is refused by the kernel: the
    plan's sticky error flag makes run(check=True) raise.  The corrupting
    hook exists only in the test build of the library, loaded by a child
    process (as tests/test_gpu_e2e.py::test_plan_device_error_flag)."""
    import subprocess
    from riptide_amd import _lib
    assert os.path.exists(_lib.TESTHOOKS_PATH), "build the test library: make -C riptide_amd/csrc"
    env = dict(os.environ, RIPTIDE_AMD_LIB=_lib.TESTHOOKS_PATH)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"REPO = {repo!r}\nGOLDEN = {os.path.join(repo, 'tests', 'golden')!r}\n" + _MISKIND_BODY
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "mis-kinded unit OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
