"""The boxcar S/N (snr.hpp:37-65) at every row shape its kernels specialise
on.  Fused (the cone kernel's epilogue: snr_epilogue / snr_rows / snr_segments
in cone_snr.hpp): bins ranges astride every breakpoint of the slot-width
variant (merge_slots), the lane-group size (snr_group) and the chunk template,
on final tiles and on whole units, with width lists on both sides of the
register window (kSnrWin) and the chunk (kSnrMaxChunk), with every select
slot of a lane in use and, across 239 | 240 and 264 | 265 bins, with widths
<= 9 (the segmented form) -- against the strict C oracle at 2e-6.  Standalone
(snr_prefix_kernel / snr_width_kernel in aux_kernels.hip): every chunk size
from 1 column per lane up, partial last blocks, lanes without columns.
"""
import numpy as np
import pytest

import inputs
from conftest import snr_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import riptide_amd
    return riptide_amd


def _scaled_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1.0)).max())


# ---------------------------------------------------------------- fused S/N
@pytest.mark.parametrize("bmin,bmax", inputs.SNR_SHAPE_RANGES, ids=[f"{a}-{b}" for a, b in inputs.SNR_SHAPE_RANGES])
def test_fused_snr_row_shapes(rt, oracle, monkeypatch, bmin, bmax):
    """One bins range astride a breakpoint of the fused S/N's instantiations
    (inputs.SNR_SHAPE_RANGES), at two sizes -- 2^16 samples: the low rungs
    take several passes, the S/N runs on final tiles; 5 bins_max + 3 samples:
    every transform one whole unit of about 5 rows -- and three width lists
    (inputs.snr_shape_widths), four in the ranges that meet 240-264 bins: a
    list of widths <= 9 there, the only plans whose 240-264-bin rows take the
    segmented S/N (snr_segments; any wider width keeps the window paths), so
    236-241 and 262-275 run rows on both sides of 239 | 240 and 264 | 265 in
    one plan.  On the tiles size that plan's final tiles are the 64-row
    blocks of the segmented form (it moves other bytes than the plan built
    with the feature bit off, RIPTIDE_AMD_CONE_FLAGS=7, which must give the
    same S/N bit for bit); the whole units have <= 64 rows as they are.
    A batch of three distinct trials with a pulse
    train of a period inside the range: trial 0 against the strict C oracle
    on the same series (periods and foldbins equal, S/N within 2e-6 of
    max(|S/N|, 1): test_periodogram_golden's bound, the two make the same
    additions per step) and bit-identical to the host entry
    libcpp.periodogram; trials 1 and 2 bit-identical to their own batch-1
    runs through the same plan (the later trials of a workgroup's trial loop).
    Worst scaled error against the oracle over the whole sweep, measured on an
    MI355X: 0.0 (every S/N value of every range, size and width list
    identical to the oracle's)."""
    import torch
    from riptide_amd import engine, generate_width_trials, libcpp
    tsamp = inputs.SNR_SHAPE_TSAMP
    wlists = inputs.snr_shape_widths(bmin, bmax, generate_width_trials(bmin, ducy_max=0.2))
    assert len(wlists["all32"]) == 32 and max(wlists["mixed"]) == bmin - 1
    assert all(1 <= w < bmin for ws in wlists.values() for w in ws)
    assert ("narrow" in wlists) == ((bmin, bmax) in ((236, 241), (262, 275)))
    assert max(wlists.get("narrow", [1])) <= 9
    # the limits of a plan (argument errors, raised before any device work):
    # 32 widths, rows of 2880 bins
    c = inputs.snr_shape_plan(bmin, bmax, 1 << 16)
    with pytest.raises(ValueError, match="at most 32 trial widths"):
        engine.PeriodogramPlan(c["n"], tsamp, [1] * 33, c["pmin"], c["pmax"], bmin, bmax)
    with pytest.raises(ValueError, match="bins_max too large"):
        engine.PeriodogramPlan(c["n"], tsamp, [1], c["pmin"], c["pmax"], bmin, 2881)
    cases = []
    for kind, n in inputs.snr_shape_sizes(bmax).items():
        c = inputs.snr_shape_plan(bmin, bmax, n)
        # pulse periods inside the first rung's span of the range
        xs = np.stack([inputs.with_signal(n, tsamp, 100 * bmin + s, (bmin + (0.3 + 0.2 * s) * (bmax - bmin)) * tsamp * 1.003,
                                          8.0) for s in range(3)])
        for wname, ws in wlists.items():
            w = np.asarray(ws, dtype=np.uint64)
            ref = oracle.periodogram(xs[0], tsamp, w, c["pmin"], c["pmax"], bmin, bmax)
            # before any GPU time is spent
            assert np.isfinite(ref[2]).all(), (kind, wname)
            cases.append((kind, c, xs, wname, w, ref))
    worst = 0.0
    for kind, c, xs, wname, w, (operiods, ofoldbins, osnr) in cases:
        tag = f"{kind} n={c['n']} widths={wname}"
        args = (c["pmin"], c["pmax"], bmin, bmax)
        plan = engine.PeriodogramPlan(c["n"], tsamp, w, *args)
        st = plan.stats()
        if kind == "tiles":
            assert st["items"] > st["transforms"], tag
        else:
            assert st["items"] == st["transforms"], tag
        periods, foldbins = plan.grid()
        assert set(range(bmin, bmax + 1)) <= set(foldbins.tolist()), tag
        assert np.array_equal(periods, operiods) and np.array_equal(foldbins, ofoldbins), tag
        d = torch.from_numpy(xs).cuda()
        batch = plan.run(d, check=True).cpu().numpy()
        err = _scaled_err(batch[0], osnr)
        worst = max(worst, err)
        print(f"fused S/N bins {bmin}-{bmax} {tag}: L={periods.size} W={w.size} scaled err vs oracle {err:.3e}")
        ok, msg = snr_close(batch[0], osnr, rtol=2e-6)
        if not ok:
            bad = np.abs(batch[0].astype(np.float64) - osnr) / np.maximum(np.abs(osnr), 1.0)
            r, iw = np.unravel_index(int(np.argmax(bad)), bad.shape)
            first = int(np.argmax(bad.max(axis=1) > 2e-6))
            msg += (f"; worst at row {r} (bins {foldbins[r]}) width {int(w[iw])}: {batch[0][r, iw]!r} vs {osnr[r, iw]!r};"
                    f" first bad row {first} (bins {foldbins[first]})")
        assert ok, f"{tag}: {msg}"
        for b in (1, 2):
            single = plan.run(d[b:b + 1].contiguous(), check=True).cpu().numpy()[0]
            assert np.array_equal(batch[b], single), f"{tag}: trial {b} of the batch differs from its batch-1 run"
        hp, hf, hsnr = libcpp.periodogram(xs[0], tsamp, w, *args)
        assert np.array_equal(hp, operiods) and np.array_equal(hf, ofoldbins), tag
        assert np.array_equal(batch[0], hsnr), f"{tag}: the device API differs from the host entry"
        if wname == "narrow":
            # the same plan with the segmented S/N's feature bit off: window-path
            # final tiles (no 64-row cap), the same S/N
            monkeypatch.setenv("RIPTIDE_AMD_CONE_FLAGS", "7")
            try:
                wplan = engine.PeriodogramPlan(c["n"], tsamp, w, *args)
                wbatch = wplan.run(d, check=True).cpu().numpy()
            finally:
                monkeypatch.delenv("RIPTIDE_AMD_CONE_FLAGS")
            if kind == "tiles":
                assert wplan.stats()["moved_bytes"] != st["moved_bytes"], f"{tag}: no segmented final tiles"
            assert np.array_equal(batch, wbatch), f"{tag}: segmented S/N differs from the window path"
    print(f"fused S/N bins {bmin}-{bmax}: worst scaled err vs oracle {worst:.3e}")


# ---------------------------------------------------------------- standalone kernels
def _snr_float64(x, widths, stdnoise):
    """snr.hpp:37-65 in float64: the prefix sum of the doubled row, the
    maximum of c[i + w] - c[i] over the row's starts, the h / b formula."""
    x = np.asarray(x, dtype=np.float64)
    rows, cols = x.shape
    c = np.cumsum(np.concatenate([x, x], axis=1), axis=1)
    total = c[:, cols - 1]
    out = np.empty((rows, len(widths)))
    for iw, w in enumerate(widths):
        dmax = (c[:, w:w + cols] - c[:, :cols]).max(axis=1)
        h = np.sqrt((cols - w) / (cols * w))
        b = w / (cols - w) * h
        out[:, iw] = ((h + b) * dmax - b * total) / stdnoise
    return out


SNR_COLS = (2, 3, 5, 63, 64, 65, 127, 128, 129, 1000, 4097, 70001)
SNR_ROWS = (1, 3, 5, 257)


def test_boxcar_snr_shapes(rt, oracle):
    """boxcar_snr (snr_prefix_kernel + snr_width_kernel: one wave per row,
    four rows per block, chunks of ceil(cols / 64) columns per lane) at chunk
    sizes 1, 2, 3, 16, 65 and 1094, column counts on both sides of a multiple
    of 64 (lanes without columns, a short last chunk) and row counts that
    leave a partial last block; widths 1, 2, 3, cols / 3, cols / 2, cols - 2
    and cols - 1 (the wrap c[k - cols] + sum for nearly every start).
    A: unit noise -- within 2e-6 of the strict C oracle, and within
    BASELINE.json's 1e-4 of the float64 restatement (the float32 reference
    arithmetic alone is within 4.0e-6 of it on these inputs).  B: the same noise
    + 5.0, so the prefix values are large and the wrap addition rounds --
    against the oracle only (the reference's own float32 prefix departs from
    float64 by up to 1e-2 at 70001 columns).
    Measured on an MI355X: worst scaled error A 0.0 against the oracle (all
    values identical) and 4.0e-6 against float64, B 0.0."""
    worst = {"A": 0.0, "A64": 0.0, "B": 0.0}
    for cols in SNR_COLS:
        widths = sorted({w for w in (1, 2, 3, cols // 3, cols // 2, cols - 2, cols - 1) if 1 <= w <= cols - 1})
        for rows in ((2,) if cols == 70001 else SNR_ROWS):
            noise = np.random.RandomState(1000 * rows + cols % 997).normal(size=(rows, cols)).astype(np.float32)
            for name, x in (("A", noise), ("B", noise + np.float32(5.0))):
                tag = f"input {name} rows={rows} cols={cols} widths={widths}"
                out = rt.boxcar_snr(x, widths, 1.7)
                assert out.shape == (rows, len(widths)) and out.dtype == np.float32
                ref = oracle.snr2(x, widths, 1.7)
                assert np.isfinite(ref).all(), tag
                worst[name] = max(worst[name], _scaled_err(out, ref))
                ok, msg = snr_close(out, ref, rtol=2e-6)
                assert ok, f"{tag}: {msg}"
                if name == "A":
                    ref64 = _snr_float64(x, widths, 1.7)
                    worst["A64"] = max(worst["A64"], _scaled_err(out, ref64))
                    ok, msg = snr_close(out, ref64)
                    assert ok, f"{tag} (float64): {msg}"
    print("boxcar_snr worst scaled err: A vs oracle {A:.3e}, A vs float64 {A64:.3e}, B vs oracle {B:.3e}".format(**worst))
