"""Time the dedispersion kernels (engine.dedisperse_device) on one resident
block of synthetic uint8 data generated on the device: by default 1024
channels x 2^22 samples at 256 DMs of a 1.2-1.5 GHz band sampled at 256 us.
Between two HIP events per call (transpose + shift-and-add, output and
workspace preallocated); one warm-up, then the median of --repeats calls.

Reports ms per DM trial, channel-samples/s, algorithmic bytes/s (block read
once, output written once) and the ratio of the per-trial time to the
per-trial search time of BENCH_r06.json (cfg2: ms_per_step over 16 trials).
--zero-dm adds the same call with the zero-DM filter (row mean + float
transpose + float sum) and the row-mean kernel alone; --stats adds
engine.channel_stats_device alone.  Both report their time next to the plain
call's, the row-mean and statistics kernels also as GB/s against the block's
bytes (each reads the block once).
--nbits 1, 2, 4 or 16 times the same shape as packed rows instead (the unpack
inside the transpose): 4096 rows of uniform values packed on the host with
reading.pack_samples and repeated down the block.  --stream adds the streamed
dedisperse_filterbank of a file of the same rows (written to --stream-dir,
page cache warm), the upload included.
--bands N adds engine.dedisperse_bands_device on the same block and DM list
with the N sub-bands of dedispersion.band_edges: the same reads and additions
as the plain call, N times its output.  Reported next to the plain call's time
with both outputs' bytes and the time the plain call would take for the extra
output at the bandwidth it achieved.
--block-mask writes the block to a file in --stream-dir and times
dedisperse_filterbank on it with and without a block mask (5 % of the cells of
--block-len samples flagged, the same build's plain call beside it,
alternating), the resident-block call with and without it (kernels only,
alternating too; with --zero-dm also the zero-DM call and the row mean alone),
and rfi.block_stats; a mask that flags nothing must give the plain call's bits.
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
    ap.add_argument("--zero-dm", action="store_true", help="also time the call with the zero-DM filter")
    ap.add_argument("--stats", action="store_true", help="also time the channel statistics")
    ap.add_argument("--nbits", type=int, default=0, choices=[0, 1, 2, 4, 16],
                    help="time packed rows of this width instead of 8-bit samples")
    ap.add_argument("--bands", type=int, default=0, help="also time the sub-band call with this many bands")
    ap.add_argument("--stream", action="store_true", help="also time dedisperse_filterbank on a file of the block")
    ap.add_argument("--stream-dir", default="/tmp")
    ap.add_argument("--block-mask", action="store_true",
                    help="also time dedisperse_filterbank and the resident call with and without a block mask, and "
                         "rfi.block_stats, on a file of the block")
    ap.add_argument("--block-len", type=int, default=2048, help="time samples of a block of --block-mask")
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")
    import torch
    import bench
    from riptide_amd import engine
    from riptide_amd.dedispersion import band_edges, dedisperse_filterbank, dispersion_delays
    from riptide_amd.reading import open_filterbank, pack_samples, unpack_samples, write_sigproc

    nchans, nsamp, ndm, tsamp = args.nchans, 1 << args.log2_nsamp, args.ndm, 256e-6
    freqs = 1500.0 - (300.0 / nchans) * np.arange(nchans)
    dms = np.linspace(0.0, args.dm_max, ndm)
    delays, max_delay = dispersion_delays(freqs, dms, tsamp)
    nout = nsamp - max_delay
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    nbits = args.nbits or None
    tile_rows = min(4096, nsamp)
    if nbits is None:
        block = torch.randint(0, 256, (nsamp, nchans), dtype=torch.uint8, device="cuda", generator=gen)
    else:
        vals = np.random.RandomState(0).randint(0, 1 << nbits, size=(tile_rows, nchans))
        block = torch.from_numpy(pack_samples(vals, nbits)).cuda().repeat(nsamp // tile_rows, 1)
    dname = "uint8" if nbits is None else f"u{nbits}"

    def rows(t0, n):
        """The values of rows [t0, t0 + n) as int64 on the device."""
        if nbits is None:
            return block[t0:t0 + n].to(torch.int64)
        return torch.from_numpy(unpack_samples(block[t0:t0 + n].cpu().numpy(), nbits, nchans).astype(np.int64)).cuda()
    d_delays = torch.from_numpy(delays.astype(np.int32)).cuda()
    out = torch.empty((ndm, nout), dtype=torch.float32, device="cuda")
    ws = torch.empty(engine.dedisperse_workspace_bytes(dname, nsamp, nchans), dtype=torch.uint8, device="cuda")

    def run():
        engine.dedisperse_device(block, d_delays, max_delay, out=out, workspace=ws, nbits=nbits)

    run()
    torch.cuda.synchronize()
    # spot check of the warm-up's result against the definition: 4 DMs x 64 outputs
    dm_rows = [0, ndm // 3, ndm // 2, ndm - 1]
    t_chk = min(12345, nout - 64)
    times = torch.arange(t_chk, t_chk + 64, device="cuda")
    idx = torch.from_numpy(delays[dm_rows]).cuda()[:, None, :] + times[None, :, None]
    win = rows(t_chk, min(max(4096, 64 + max_delay), nsamp - t_chk))     # the rows the checks read
    picked = win[idx - t_chk, torch.arange(nchans, device="cuda")[None, None, :]]
    ref = picked.sum(dim=2)
    got = out[dm_rows, t_chk:t_chk + 64].to(torch.float64)
    # exact, but for 16-bit data: float32 additions in channel order
    bound = nchans * 2.0 ** -24 * ref.to(torch.float64) if nbits == 16 else 0.0
    assert bool(((got - ref.to(torch.float64)).abs() <= bound).all()), "dedisperse_device differs from its definition"
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        ms = []
        for _ in range(args.repeats):
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    ms = timed(run)
    med = float(np.median(ms))
    block_bytes = block.numel()
    extra = {}
    if args.zero_dm:
        zws = torch.empty(engine.dedisperse_workspace_bytes(dname, nsamp, nchans, zero_dm=True), dtype=torch.uint8,
                          device="cuda")
        mean = torch.empty(nsamp, dtype=torch.float32, device="cuda")

        def run_zero_dm():
            engine.dedisperse_device(block, d_delays, max_delay, out=out, workspace=zws, zero_dm=True, nbits=nbits)

        def run_mean():
            engine.zero_dm_mean_device(block, out=mean, nbits=nbits)

        run_zero_dm()
        run_mean()
        torch.cuda.synchronize()
        # spot check against the definition: the mean series bit for bit, the
        # sums within nchans * 2^-24 * sum |y| of the float64 sums of x - m
        m_ref = (win.sum(dim=1).to(torch.float64) / nchans).to(torch.float32)
        assert torch.equal(mean[t_chk:t_chk + win.shape[0]], m_ref), "zero_dm_mean_device differs from its definition"
        y = picked.to(torch.float64) - mean[idx].to(torch.float64)
        err = (out[dm_rows, t_chk:t_chk + 64].to(torch.float64) - y.sum(dim=2)).abs()
        assert bool((err <= nchans * 2.0 ** -24 * y.abs().sum(dim=2)).all()), "zero-DM sums differ from the definition"
        zms, mms = timed(run_zero_dm), timed(run_mean)
        zmed, mmed = float(np.median(zms)), float(np.median(mms))
        extra.update({"zero_dm_call_ms_median": zmed, "zero_dm_call_ms_min": float(np.min(zms)),
                      "zero_dm_call_ms_max": float(np.max(zms)), "zero_dm_ms_per_dm_trial": zmed / ndm,
                      "zero_dm_to_plain_ratio": zmed / med,
                      "zero_dm_workspace_bytes": zws.numel(),
                      "row_mean_ms_median": mmed, "row_mean_block_gb_per_s": block_bytes / (mmed * 1e-3) / 1e9})
    if args.stats:
        acc = torch.zeros((2, nchans), dtype=torch.float64, device="cuda")
        sws = torch.empty(engine.channel_stats_workspace_bytes(nsamp, nchans), dtype=torch.uint8, device="cuda")

        def run_stats():
            engine.channel_stats_device(block, acc, workspace=sws, nbits=nbits)

        run_stats()
        torch.cuda.synchronize()
        if nbits is None:
            part, reps = block[:, :8].to(torch.int64), 1
        else:       # the block is its first tile_rows rows, repeated
            part, reps = rows(0, tile_rows)[:, :8], nsamp // tile_rows
        assert torch.equal(acc[0, :8].to(torch.int64), part.sum(dim=0) * reps), "channel sums differ"
        assert torch.equal(acc[1, :8].to(torch.int64), (part * part).sum(dim=0) * reps), "channel sums of squares differ"
        sms = timed(run_stats)
        smed = float(np.median(sms))
        extra.update({"stats_ms_median": smed, "stats_ms_min": float(np.min(sms)), "stats_ms_max": float(np.max(sms)),
                      "stats_block_gb_per_s": block_bytes / (smed * 1e-3) / 1e9})
    if args.bands:
        d_bands = torch.from_numpy(band_edges(nchans, args.bands).view(np.int32)).cuda()
        bout = torch.empty((ndm, args.bands, nout), dtype=torch.float32, device="cuda")

        def run_bands():
            engine.dedisperse_bands_device(block, d_delays, max_delay, d_bands, out=bout, workspace=ws, nbits=nbits)

        run_bands()
        torch.cuda.synchronize()
        if nbits != 16:     # integer sums: the bands of a partition add up to the plain call's row exactly
            parts = bout[dm_rows, :, t_chk:t_chk + 64].to(torch.float64).sum(dim=1)
            assert torch.equal(parts, got), "the sub-band sums do not add up to the plain call's"
        bms = timed(run_bands)
        bmed = float(np.median(bms))
        plain_rate = (block_bytes + out.numel() * 4) / (med * 1e-3)     # bytes/s the plain call achieved
        extra.update({"bands": args.bands, "bands_call_ms_median": bmed, "bands_call_ms_min": float(np.min(bms)),
                      "bands_call_ms_max": float(np.max(bms)), "bands_output_bytes": bout.numel() * 4,
                      "plain_output_bytes": out.numel() * 4, "bands_to_plain_ratio": bmed / med,
                      "plain_plus_extra_output_ms": med + (bout.numel() - out.numel()) * 4 / plain_rate * 1e3})
        del bout
    if args.stream:
        # the same rows as a file, streamed in the default gulps: upload + kernels
        fname = os.path.join(args.stream_dir, f"bench_dedisperse_{dname}.fil")
        header = {"tsamp": tsamp, "nbits": nbits or 8, "fch1": float(freqs[0]), "foff": float(freqs[1] - freqs[0]),
                  "nchans": nchans, "nifs": 1}
        host_rows = block.cpu().numpy()
        write_sigproc(fname, host_rows.ravel() if nbits else host_rows, header)
        del host_rows
        fb = open_filterbank(fname)
        first = dedisperse_filterbank(fb, dms)
        torch.cuda.synchronize()
        assert torch.equal(first, out if not (args.zero_dm or args.stats) else first), "streamed result differs"
        del first
        sms = []
        for _ in range(args.repeats):
            a.record()
            res = dedisperse_filterbank(fb, dms)
            b.record()
            b.synchronize()
            sms.append(a.elapsed_time(b))
            del res
        os.remove(fname)
        extra.update({"stream_ms_median": float(np.median(sms)), "stream_ms_min": float(np.min(sms)),
                      "stream_ms_max": float(np.max(sms)), "stream_file_bytes": block_bytes})
    if args.block_mask:
        # the same rows as a file: dedisperse_filterbank with and without a block
        # mask (blocks of --block-len samples, 5 % of the cells flagged at
        # random, the fill the channels' means), the resident-block call with
        # and without it, and rfi.block_stats (upload + kernels + download)
        import time
        from riptide_amd import rfi
        fname = os.path.join(args.stream_dir, f"bench_blockmask_{dname}.fil")
        header = {"tsamp": tsamp, "nbits": nbits or 8, "fch1": float(freqs[0]), "foff": float(freqs[1] - freqs[0]),
                  "nchans": nchans, "nifs": 1}
        host_rows = block.cpu().numpy()
        write_sigproc(fname, host_rows.ravel() if nbits else host_rows, header)
        del host_rows
        fb = open_filterbank(fname)
        blen = args.block_len
        stats = rfi.block_stats(fb, block_len=blen)      # warm-up
        st_ms = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            stats = rfi.block_stats(fb, block_len=blen)
            st_ms.append((time.perf_counter() - t0) * 1e3)
        cells = np.random.RandomState(1).rand(stats.sum.shape[0], nchans) < 0.05
        bm = rfi.BlockMask(cells, blen, stats.sum.sum(axis=0) / stats.nsamp)
        clear = rfi.BlockMask(np.zeros_like(cells), blen, bm.fill)
        plain_first = dedisperse_filterbank(fb, dms)
        assert torch.equal(dedisperse_filterbank(fb, dms, block_mask=clear), plain_first), \
            "a block mask that flags nothing changes the result"
        del plain_first
        torch.cuda.synchronize()
        pms, mms = [], []
        for _ in range(args.repeats):      # alternating, so drift falls on both alike
            for kw, into in (({}, pms), ({"block_mask": bm}, mms)):
                a.record()
                res = dedisperse_filterbank(fb, dms, **kw)
                b.record()
                b.synchronize()
                into.append(a.elapsed_time(b))
                del res
        os.remove(fname)
        d_bm = engine.DeviceBlockMask(torch.from_numpy(cells.astype(np.uint8)).cuda(),
                                      torch.from_numpy(bm.typed_fill(fb)).cuda(), blen)

        def run_masked():
            engine.dedisperse_device(block, d_delays, max_delay, out=out, workspace=ws, nbits=nbits, block_mask=d_bm)

        def alternating(plain_fn, masked_fn):
            """(plain ms, masked ms), one call of each in turn."""
            masked_fn()
            torch.cuda.synchronize()
            pl, mk = [], []
            for _ in range(args.repeats):
                for fn, into in ((plain_fn, pl), (masked_fn, mk)):
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    into.append(a.elapsed_time(b))
            return pl, mk

        rpl, rms = alternating(run, run_masked)
        if args.zero_dm:
            # the zero-DM call and the row mean alone, with and without the mask
            def run_zero_dm_masked():
                engine.dedisperse_device(block, d_delays, max_delay, out=out, workspace=zws, zero_dm=True, nbits=nbits,
                                         block_mask=d_bm)

            def run_mean_masked():
                engine.zero_dm_mean_device(block, out=mean, nbits=nbits, block_mask=d_bm)

            zpl, zmk = alternating(run_zero_dm, run_zero_dm_masked)
            mpl, mmk = alternating(run_mean, run_mean_masked)
            extra.update({"zero_dm_resident_plain_ms_median": float(np.median(zpl)),
                          "zero_dm_resident_masked_ms_median": float(np.median(zmk)),
                          "zero_dm_resident_masked_ms_min": float(np.min(zmk)),
                          "zero_dm_resident_masked_ms_max": float(np.max(zmk)),
                          "zero_dm_resident_masked_to_plain_ratio": float(np.median(zmk) / np.median(zpl)),
                          "row_mean_plain_ms_median": float(np.median(mpl)),
                          "row_mean_masked_ms_median": float(np.median(mmk)),
                          "row_mean_masked_ms_min": float(np.min(mmk)), "row_mean_masked_ms_max": float(np.max(mmk)),
                          "row_mean_masked_to_plain_ratio": float(np.median(mmk) / np.median(mpl))})
        pmed, mmed, rmed, rpmed = (float(np.median(v)) for v in (pms, mms, rms, rpl))
        extra.update({"block_len": blen, "block_mask_fraction": bm.fraction,
                      "block_mask_cells_bytes": int(cells.size),
                      "file_plain_ms_median": pmed, "file_plain_ms_min": float(np.min(pms)),
                      "file_plain_ms_max": float(np.max(pms)),
                      "file_masked_ms_median": mmed, "file_masked_ms_min": float(np.min(mms)),
                      "file_masked_ms_max": float(np.max(mms)), "file_masked_to_plain_ratio": mmed / pmed,
                      "resident_plain_ms_median": rpmed, "resident_masked_ms_median": rmed,
                      "resident_masked_ms_min": float(np.min(rms)), "resident_masked_ms_max": float(np.max(rms)),
                      "resident_masked_to_plain_ratio": rmed / rpmed,
                      "block_stats_ms_median": float(np.median(st_ms)), "block_stats_ms_min": float(np.min(st_ms)),
                      "block_stats_ms_max": float(np.max(st_ms))})
    with open(os.path.join(REPO, "BENCH_r06.json")) as f:
        search_ms = json.load(f)["parsed"]["ms_per_step"] / 16.0
    result = {"nchans": nchans, "nsamp": nsamp, "ndm": ndm, "tsamp": tsamp, "dm_max": float(dms[-1]),
              "max_delay": max_delay, "nout": nout, "dtype": dname, "repeats": args.repeats,
              "call_ms_median": med, "call_ms_min": float(np.min(ms)), "call_ms_max": float(np.max(ms)),
              "ms_per_dm_trial": med / ndm,
              "channel_samples_per_s": ndm * nout * nchans / (med * 1e-3),
              "algorithmic_bytes_per_s": (block_bytes + ndm * nout * 4) / (med * 1e-3),
              "search_ms_per_trial_bench_r06_cfg2": search_ms,
              "dedisperse_to_search_ratio": (med / ndm) / search_ms,
              "source_digest": bench.source_digest(), "device": torch.cuda.get_device_name(0)}
    if "zero_dm_ms_per_dm_trial" in extra:
        extra["zero_dm_to_search_ratio"] = extra["zero_dm_ms_per_dm_trial"] / search_ms
    result.update(extra)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
