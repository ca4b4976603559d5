"""Multi-GPU DM-trial dispatcher: the replacement of rffa's CPU worker pool
(riptide/pipeline/worker_pool.py:10-70) with the same contract: a list of DM
trials in, the flat List[Peak] of every trial and search range out, in trial
order and, within a trial, in range order (WorkerPool.process_fname_list,
worker_pool.py:35-45, flattens its Pool.map results the same way).

One process per GPU (torch.distributed, backend "nccl" = RCCL on ROCm, or
"gloo" for CPU tests).  Trials are independent, so they are partitioned
statically (round-robin by index) with no data-path collective; each rank
batches its trials through the device-resident engine (dereddening +
normalisation once per trial, then one periodogram per search range, exactly
as WorkerPool.process_fname does) and device peak detection, and the
per-rank peak lists -- tagged with their trial index -- are gathered once at
the end (KB-scale, latency-bound) and put back in trial order.
"""
import contextlib
import itertools
import logging
import os
import typing

import numpy as np

from .peak_detection import Peak

log = logging.getLogger("riptide.dispatch")


class Trial(typing.NamedTuple):
    """One dedispersed time series to search."""
    data: np.ndarray          # samples as stored (float32, or uint8 / int8 8-bit data)
    tsamp: float
    metadata: dict            # must hold 'dm' (None allowed), like riptide Metadata


def shard(n_items, rank, world):
    """Indices of the trials owned by `rank`: round-robin, so every rank gets
    a near-equal share and consecutive DMs spread over the GPUs."""
    return list(range(rank, n_items, world))


def _group_by_shape(samples, tsamps):
    """{(length, tsamp): [indices]} in first-seen order (device batches need
    one series length and one sampling time)."""
    groups = {}
    for i, (x, ts) in enumerate(zip(samples, tsamps)):
        groups.setdefault((int(np.asarray(x).size), float(ts)), []).append(i)
    return groups


def _pipelined(steps, detect):
    """The slice pipeline of every search below: `steps` yields (tag, pending),
    each made by queuing one slice's device work, and item k + 1 is pulled --
    queued -- before detect runs on item k's pending: enqueue 0, enqueue 1,
    detect 0, enqueue 2, detect 1, ..., detect n - 1, the device busy through
    every detection's host stages.  Yields (tag, detected) in order."""
    steps = iter(steps)
    cur = next(steps, None)
    while cur is not None:
        nxt = next(steps, None)
        yield cur[0], detect(cur[1])
        cur = nxt


@contextlib.contextmanager
def _dedispersed(fb, dms, device, batch, **kwargs):
    """Inside the scope `device` (None, an int or a torch.device) is the
    current one and the file is dedispersed there at the trial DMs
    (dedispersion.dedisperse_filterbank, which takes kwargs): yields (series
    [ndm, nout] on the device, every trial's metadata, the [b0, b1) slices of
    `batch` DMs)."""
    import torch
    from ._args import resolve_device
    from .dedispersion import dedisperse_filterbank
    dev = resolve_device(device)
    with torch.cuda.device(dev):
        series = dedisperse_filterbank(fb, dms, device=dev, **kwargs)
        yield (series, [fb.metadata(dm) for dm in dms],
               [(b0, min(b0 + batch, len(dms))) for b0 in range(0, len(dms), batch)])


class EngineSearcher:
    """Batched GPU search of DM trials: the hot path.  For every search range:
    one compiled periodogram plan per (length, tsamp, range) and device peak
    detection (riptide_amd.peaks.PeakFinder); only the peaks leave the device.

    Calling it on a list of Trial returns one peak list per trial, in the
    order given (each in range order, as WorkerPool.process_fname)."""

    def __init__(self, deredden_params, range_confs, device=None, batch=8, check=True, device_cluster=None):
        self.deredden_params = dict(deredden_params)
        self.range_confs = list(range_confs)
        self.device = device
        self.batch = int(batch)
        self.check = bool(check)
        # clustering and the argmax per cluster on the device (PeakFinder's
        # device_cluster); None: the A/B switch RIPTIDE_AMD_DEVICE_PEAKS
        self.device_cluster = (bool(os.environ.get("RIPTIDE_AMD_DEVICE_PEAKS")) if device_cluster is None
                               else bool(device_cluster))
        self._plans = {}
        self._finders = {}
        self._ws = {}
        self._side = {}

    def _plan(self, n, tsamp, conf):
        from . import engine
        kw = conf["ffa_search"]
        key = (n, tsamp, tuple(sorted(kw.items())))
        if key not in self._plans:
            self._plans[key] = engine.PeriodogramPlan.for_search(
                n, tsamp, kw["period_min"], kw["period_max"], kw.get("bins_min", 240), kw.get("bins_max", 260),
                ducy_max=kw.get("ducy_max", 0.2), wtsp=kw.get("wtsp", 1.5), device=self.device)
        return self._plans[key]

    def _finder(self, plan, tobs, conf):
        from .peaks import PeakFinder
        kw = conf.get("find_peaks", {}) or {}
        key = (id(plan), tobs, tuple(sorted(kw.items())))
        if key not in self._finders:
            self._finders[key] = PeakFinder(plan, tobs, device_cluster=self.device_cluster, **kw)
        return self._finders[key]

    def _workspace(self, plan, B):
        import torch
        need = plan.workspace_bytes(B)
        ws = self._ws.get(id(plan))
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=plan.device)
            self._ws[id(plan)] = ws
        return ws

    def _side_stream(self, dev):
        import torch
        if dev not in self._side:
            self._side[dev] = torch.cuda.Stream(device=dev)
        return self._side[dev]

    def search_device(self, raw, tsamp, metadatas):
        """Peaks of every trial of a device batch raw [B, N] (float32): one
        list per trial, in range order (WorkerPool.process_fname)."""
        return self._detect(self._enqueue(raw, tsamp, metadatas))

    def _enqueue(self, raw, tsamp, metadatas):
        """Queue a device batch's deredden + normalise and every range's
        periodogram on the current stream; returns the pending batch for
        _detect.  Nothing here waits for the device."""
        return self._enqueue_series(self._normalise(raw, tsamp), tsamp, [m.get("dm") for m in metadatas])

    def _normalise(self, raw, tsamp):
        """deredden + normalise of a device batch, queued on the current stream."""
        from . import engine
        ws = int(round(self.deredden_params["rmed_width"] / tsamp))
        return engine.deredden_normalise(raw, ws, self.deredden_params["rmed_minpts"])

    def _enqueue_series(self, x, tsamp, dms):
        """_enqueue behind the normalisation: every range's periodogram of the
        normalised batch x, one row per entry of dms."""
        import torch
        B, n = x.shape
        main = torch.cuda.current_stream(x.device)
        if os.environ.get("RIPTIDE_AMD_PEAKS_SERIAL"):
            return {"serial": True, "x": x, "n": n, "tsamp": tsamp, "dms": dms}
        runs = []
        for conf in self.range_confs:
            plan = self._plan(n, tsamp, conf)
            snr = plan.run(x, workspace=self._workspace(plan, B))
            ev = torch.cuda.Event()
            ev.record(main)
            runs.append((conf, plan, snr, ev))
        return {"serial": False, "runs": runs, "n": n, "tsamp": tsamp, "dms": dms, "B": B, "device": x.device, "x": x}

    def _detect(self, pend):
        """Peak detection of a pending batch, range by range, on a side
        stream: each range's detection starts once its periodogram is done
        (an event), so its host stages (the order statistics' polyfits, the
        selected rows' clustering) overlap the periodograms queued after it
        -- the later ranges', and with submit_samples the next batch's --
        instead of leaving the GPU idle.  Same kernels on the same data:
        same peaks."""
        n, tsamp, dms = pend["n"], pend["tsamp"], pend["dms"]
        if pend["serial"]:
            # A/B (RIPTIDE_AMD_PEAKS_SERIAL): each range's detection right
            # after its periodogram, on the same stream, nothing queued ahead
            x = pend["x"]
            out = [[] for _ in range(x.shape[0])]
            for conf in self.range_confs:
                plan = self._plan(n, tsamp, conf)
                snr = plan.run(x, workspace=self._workspace(plan, x.shape[0]))
                if self.check:
                    plan.check()
                for b, (peaks, _) in enumerate(self._finder(plan, n * tsamp, conf)(snr, dms=dms)):
                    out[b].extend(peaks)
            return out
        out = [[] for _ in range(pend["B"])]
        side = self._side_stream(pend["device"])
        for conf, plan, snr, ev in pend["runs"]:
            side.wait_event(ev)
            snr.record_stream(side)
            for b, (peaks, _) in enumerate(self._finder(plan, n * tsamp, conf)(snr, dms=dms, stream=side)):
                out[b].extend(peaks)
        if self.check:
            for _, plan, _, _ in pend["runs"]:
                # device error flag, read on the side stream: ordered after
                # this batch's periodograms (the events), not waiting for
                # what is queued behind them; RuntimeError if a unit broke
                # its budget
                plan.check(side)
        return out

    def submit_samples(self, samples, tsamps, metadatas, uploaded=None):
        """search_samples in two halves: uploads and periodograms of every
        device batch queued now, peak detection when the returned callable is
        called (-> per-trial peak lists in input order).  A caller that
        submits chunk k + 1 before collecting chunk k keeps the device busy
        through chunk k's host stages (GpuWorkerPool.search_chunks); device
        batches within one call are pipelined the same way.  `uploaded()`, if
        given, is called once the last batch's upload is queued: the host
        samples may be reused after the device work queued at that moment (an
        event)."""
        from .reading import upload_samples
        batches = []
        for (n, tsamp), idx in _group_by_shape(samples, tsamps).items():
            for b0 in range(0, len(idx), self.batch):
                batches.append((tsamp, idx[b0:b0 + self.batch]))
        per = [None] * len(samples)

        def steps():
            for k, (tsamp, chunk) in enumerate(batches):
                x = upload_samples([samples[i] for i in chunk], device=self.device)
                if k + 1 == len(batches) and uploaded is not None:
                    uploaded()
                yield chunk, self._enqueue(x, tsamp, [metadatas[i] for i in chunk])

        queued = steps()
        first = list(itertools.islice(queued, 1))       # the first batch is queued now, the rest by collect()
        if not batches and uploaded is not None:
            uploaded()
        pipe = _pipelined(itertools.chain(first, queued), self._detect)

        def collect():
            for chunk, peaks in pipe:
                for i, p in zip(chunk, peaks):
                    per[i] = p
            return per

        return collect

    def search_samples(self, samples, tsamps, metadatas):
        """Per-trial peak lists of host sample arrays (float32 or 8-bit, as
        stored): grouped by (length, tsamp), uploaded in device batches
        (8-bit data converted on the device), results in input order."""
        return self.submit_samples(samples, tsamps, metadatas)()

    def search_filterbank(self, fb, dms, mask=None, nout=None, kdm=None, zero_dm=False, pulses=None,
                          block_mask=None, inject=None):
        """Dedisperse a reading.Filterbank or PackedFilterbank at the trial DMs on the device
        (dedispersion.dedisperse_filterbank) and search every series: one peak
        list per DM, in the order given (the __call__ contract).  The series
        never leave the device: they go to _enqueue / _detect in slices of
        `batch` DMs, slice k + 1 queued before slice k's detection as in
        submit_samples.  Each trial's metadata is the file's with `dm` set.
        `nout` cuts every series to its first nout samples (the length a
        longer DM list would leave: search_filterbank of this module); `kdm`
        is the dispersion constant of the delay table (default:
        dedispersion.KDM); `zero_dm` puts the zero-DM filter in front of the
        sum (dedispersion.dedisperse_filterbank; rfi.channel_mask builds a
        `mask` from the file's channel statistics); `block_mask` (a
        rfi.BlockMask, from rfi.block_mask(rfi.block_stats(fb))) replaces the
        samples of its flagged (time block, channel) cells by the channel's
        fill as the file is read; `inject` (an injection.InjectionTables, or
        (tables, seed)) adds synthetic signals to the samples in front of all
        of that (dedispersion.dedisperse_filterbank).

        pulses: None, or a dict of single_pulse.search_pulses parameters
        (widths, threshold, radius, time_radius, dm_gap, max_events): every
        slice's normalised series then also goes through the single-pulse
        search (engine.single_pulse_device), and the return is (peak lists,
        pulses), the SinglePulse list of single_pulse.cluster_events over all
        DMs; the events behind them (series = index into dms) are kept in
        self.pulse_events."""
        from . import engine, single_pulse
        from .dedispersion import KDM
        kdm = KDM if kdm is None else float(kdm)
        dms = [float(d) for d in dms]
        kw = None if pulses is None else dict(pulses)
        if kw is not None:
            unknown = set(kw) - {"widths", "threshold", "radius", "time_radius", "dm_gap", "max_events"}
            if unknown:
                raise ValueError(f"unknown single-pulse parameters: {sorted(unknown)}")
            self.pulse_events = np.empty(0, dtype=single_pulse.EVENT_DTYPE)
        if not dms:
            return [] if kw is None else ([], [])
        per, parts = [], []
        with _dedispersed(fb, dms, self.device, self.batch, mask=mask, nout=nout, kdm=kdm, zero_dm=zero_dm,
                          block_mask=block_mask, inject=inject) as (series, metas, slices):
            each = None
            if kw is not None:
                widths = single_pulse._default_widths(kw.get("widths"), series.shape[1])

                def each(b0, pend):
                    # the single-pulse search of a slice's normalised series, right behind its periodograms
                    ev = engine.single_pulse_device(pend["x"], widths, kw.get("threshold", 8.0),
                                                    radius=kw.get("radius"), max_events=kw.get("max_events", 1 << 20))
                    parts.append(single_pulse.events_to_host(ev, b0))

            def steps():
                for b0, b1 in slices:
                    pend = self._enqueue(series[b0:b1], fb.tsamp, metas[b0:b1])
                    if each is not None:
                        each(b0, pend)
                    yield b0, pend

            for _, peaks in _pipelined(steps(), self._detect):
                per.extend(peaks)
        if kw is None:
            return per
        self.pulse_events = np.concatenate(parts)
        found = single_pulse.cluster_events(self.pulse_events, dms, fb.tsamp, time_radius=kw.get("time_radius"),
                                            dm_gap=kw.get("dm_gap", 1), widths=widths)
        return per, found

    def search_device_accel(self, raw, tsamp, metadatas, accels):
        """The acceleration search of a device batch raw [D, N] (float32), one
        dedispersed series per DM: every series at every trial acceleration of
        `accels` (m/s^2, acceleration.accel_trials).  Each series is dereddened
        and normalised once, in slices of `batch` DMs; its (DM, accel) rows,
        DM-major, are stretched by engine.resample_device in slices of at most
        `batch` rows, and every slice goes the way of a search_device batch,
        slice k + 1 queued before slice k's detection.  Returns one list of
        acceleration.AccelPeak per DM, in accel order, then range order."""
        from . import engine
        from .acceleration import AccelPeak, accel_factor
        accels = [float(a) for a in accels]
        D, A = raw.shape[0], len(accels)
        out = [[] for _ in range(D)]
        if not D or not A:
            return out
        factors = np.array([accel_factor(a, tsamp) for a in accels], dtype=np.float64)
        dms = [m.get("dm") for m in metadatas]

        def steps():
            for d0 in range(0, D, self.batch):
                d1 = min(d0 + self.batch, D)
                x = self._normalise(raw[d0:d1], tsamp)
                for r0 in range(d0 * A, d1 * A, self.batch):
                    rows = np.arange(r0, min(r0 + self.batch, d1 * A))
                    y = engine.resample_device(x, factors[rows % A], src=rows // A - d0)
                    yield rows, self._enqueue_series(y, tsamp, [dms[r // A] for r in rows])

        for rows, per in _pipelined(steps(), self._detect):
            for r, peaks in zip(rows, per):
                out[r // A].extend(AccelPeak(*p, accels[r % A]) for p in peaks)
        return out

    def search_filterbank_accel(self, fb, dms, accels, mask=None, nout=None, kdm=None, zero_dm=False,
                                block_mask=None, inject=None):
        """search_filterbank with an acceleration axis: the file dedispersed at
        the trial DMs on the device, then search_device_accel of the series.
        One list of acceleration.AccelPeak per DM, in the order given; fb, mask,
        nout, kdm, zero_dm, block_mask and inject as for search_filterbank.  With
        accels = [0.0] the peaks are search_filterbank's.  The single-pulse
        search (pulses=) is not combined with it."""
        from .dedispersion import KDM
        kdm = KDM if kdm is None else float(kdm)
        dms = [float(d) for d in dms]
        if not dms:
            return []
        with _dedispersed(fb, dms, self.device, self.batch, mask=mask, nout=nout, kdm=kdm, zero_dm=zero_dm,
                          block_mask=block_mask, inject=inject) as (series, metas, _):
            return self.search_device_accel(series, fb.tsamp, metas, accels)

    def search_filterbank_plan(self, fb, plan, mask=None, kdm=None, zero_dm=False, block_mask=None,
                               budget_bytes=None, inject=None):
        """search_filterbank over a dedispersion.DMPlan: the file is
        dedispersed once at every trial of the plan, each step decimated in
        time by its factor (dedispersion.dedisperse_filterbank_plan), and
        every step's series are searched at the step's sampling time, f *
        fb.tsamp -- plans and peak finders are cached per (length, tsamp), and
        deredden_params["rmed_width"] is in seconds.  Each step's series go to
        _enqueue in slices of `batch` DMs, pipelined across steps as the
        slices of search_filterbank are.  One peak list per DM, in plan order;
        each trial's metadata is the file's with `dm` and the step's `tsamp`.
        fb, mask, kdm, zero_dm, block_mask and inject as for search_filterbank; every
        step covers the stretch of the observation plan.dm_cover leaves.

        A plan whose series do not fit budget_bytes of device memory (default:
        dedispersion.DEFAULT_BUDGET_BYTES) at once is cut into consecutive
        slices that do (dedispersion.plan_slices), each dedispersed and
        searched in turn, one pass over the file per slice; the slices keep
        dm_cover, so the peaks do not depend on the budget.

        Out of scope: pulses= (event sample indices and
        single_pulse.cluster_events assume one sampling time), the
        acceleration axis, and bands= with decimation."""
        import torch
        from ._args import resolve_device
        from .dedispersion import DEFAULT_BUDGET_BYTES, KDM, dedisperse_filterbank_plan, plan_slices
        kdm = KDM if kdm is None else float(kdm)
        if not len(plan):
            return []
        budget = DEFAULT_BUDGET_BYTES if budget_bytes is None else int(budget_bytes)
        dev = resolve_device(self.device)
        per = []
        with torch.cuda.device(dev):
            def steps():
                for part in plan_slices(fb, plan, budget, chunk=self.batch, kdm=kdm, zero_dm=zero_dm,
                                        block_mask=block_mask):
                    series = dedisperse_filterbank_plan(fb, part, mask=mask, device=dev, kdm=kdm, zero_dm=zero_dm,
                                                        block_mask=block_mask, budget_bytes=budget, inject=inject)
                    yield from slice_steps(part, series)
                    series = None       # released before the next slice is allocated

            def slice_steps(part, series):
                for step, rows in zip(part.steps, series):
                    tsamp = fb.tsamp * step.downsamp
                    metas = []
                    for dm in step.dms:
                        md = fb.metadata(float(dm))
                        md["tsamp"] = tsamp
                        metas.append(md)
                    for b0 in range(0, len(metas), self.batch):
                        yield b0, self._enqueue(rows[b0:b0 + self.batch], tsamp, metas[b0:b0 + self.batch])

            for _, peaks in _pipelined(steps(), self._detect):
                per.extend(peaks)
        return per

    def __call__(self, trials):
        return self.search_samples([t.data for t in trials], [t.tsamp for t in trials],
                                   [t.metadata for t in trials])


def _rank_world(group):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def _gather_tagged(tagged, group, world, make=Peak):
    """All ranks' (trial index, peak tuples) lists, gathered once (KB-scale),
    in trial order, flattened to the WorkerPool contract; `make` is the peaks'
    type."""
    if world > 1:
        import torch.distributed as dist
        gathered = [None] * world
        dist.all_gather_object(gathered, tagged, group=group)
        tagged = [t for part in gathered for t in part]
    tagged.sort(key=lambda t: t[0])
    return [make(*p) for _, plist in tagged for p in plist]


def _filterbank_shard(fb_or_fname, dms, kdm, group):
    """What the filterbank searches below do first: the file opened, kdm and
    dms normalised, this rank's round-robin share `mine` of the DMs and the
    length `nout` the whole DM list leaves, nsamp minus its largest delay ([]
    and 0 without DMs).  Returns (fb, dms, kdm, world, mine, nout)."""
    from .dedispersion import KDM, check_max_delay, dispersion_delays
    from .reading import Filterbank, open_filterbank
    kdm = KDM if kdm is None else float(kdm)
    fb = fb_or_fname if isinstance(fb_or_fname, Filterbank) else open_filterbank(fb_or_fname)
    dms = [float(d) for d in dms]
    rank, world = _rank_world(group)
    if not dms:
        return fb, dms, kdm, world, [], 0
    _, max_delay = dispersion_delays(fb.freqs, dms, fb.tsamp, kdm)
    check_max_delay(max_delay, fb.nsamp)
    return fb, dms, kdm, world, shard(len(dms), rank, world), fb.nsamp - max_delay


def _gather_per_dm(mine, local, group, world, make=Peak):
    """And last: this rank's one peak list per DM of `mine`, tagged and gathered."""
    if len(local) != len(mine):
        raise RuntimeError("searcher must return one peak list per DM")
    return _gather_tagged([(i, [tuple(p) for p in plist]) for i, plist in zip(mine, local)], group, world, make)


def search_trials(trials, searcher, group=None, loader=None, chunksize=None):
    """Search this rank's share of the DM trials with `searcher` (a callable
    taking a list of Trial and returning one peak list per trial, in order)
    and gather every rank's lists.  Returns the full peak list on every
    rank, in trial order (then range order within a trial): the WorkerPool
    contract (worker_pool.py:35-45).

    `trials` is a sequence of Trial, or -- with `loader` -- the number of
    trials, `loader(i)` returning Trial i: each rank then loads only its own
    shard, `chunksize` trials at a time (default: the searcher's batch), so no
    rank ever holds the whole list."""
    rank, world = _rank_world(group)
    n = int(trials) if loader is not None else len(trials)
    get = loader if loader is not None else (lambda i: trials[i])
    mine = shard(n, rank, world)
    cs = int(chunksize or getattr(searcher, "batch", 0) or max(1, len(mine)))
    tagged = []
    for c0 in range(0, len(mine), cs):
        idx = mine[c0:c0 + cs]
        local = searcher([get(i) for i in idx])
        if len(local) != len(idx):
            raise RuntimeError("searcher must return one peak list per trial")
        tagged += [(i, [tuple(p) for p in plist]) for i, plist in zip(idx, local)]
    return _gather_tagged(tagged, group, world)


def search_files(fnames, pool, group=None, chunksize=None):
    """rffa's search stage over the ranks of one node (pipeline.py:177-189 with
    dmiter.py:231-243): each rank searches its round-robin share of the
    DM-ordered file list through `pool` (a GpuWorkerPool) in chunks of
    `chunksize` files (default: the pool's batch), the next chunk read into
    a bounded page-locked ring while the current one is on the device
    (GpuWorkerPool.search_chunks); one gather of the tagged peak lists.
    Returns the full peak list on every rank, in file order."""
    rank, world = _rank_world(group)
    fnames = list(fnames)
    mine = shard(len(fnames), rank, world)
    tagged = []
    for first, per_file in pool.search_chunks([fnames[i] for i in mine], chunksize=chunksize):
        tagged += [(mine[first + j], [tuple(p) for p in plist]) for j, plist in enumerate(per_file)]
    return _gather_tagged(tagged, group, world)


def search_filterbank(fb_or_fname, dms, searcher, group=None, mask=None, kdm=None, zero_dm=False, pulses=None,
                      block_mask=None, inject=None):
    """Search a channelised SIGPROC file (a file name, opened by
    reading.open_filterbank: 1-, 2-, 4-, 8-, 16- or 32-bit samples; or a
    Filterbank / PackedFilterbank) at the trial DMs without leaving the
    device: each rank dedisperses its round-robin share of `dms`
    (searcher.search_filterbank, an EngineSearcher) from the one file and
    searches the series in device memory; one gather of the tagged peak
    lists.  Returns the full peak list on every rank, in the order of `dms`
    (then range order within a DM): the search_trials contract.  Every rank
    cuts its series to the length the whole DM list leaves, nsamp minus the
    list's largest delay, so the result does not depend on the sharding.
    `kdm` is the dispersion constant of the delay table, on every rank
    (default: dedispersion.KDM); `zero_dm` subtracts every time sample's mean
    over the unmasked channels before the sum (the zero-DM filter);
    `block_mask` (a rfi.BlockMask) replaces the samples of its flagged (time
    block, channel) cells by the channel's fill in front of both; `inject` (an
    injection.InjectionTables, or (tables, seed)) adds synthetic signals to the
    samples in front of all three, the same on every rank.

    pulses: None, or a dict of single_pulse.search_pulses parameters: every
    rank then also runs the single-pulse search on its normalised series
    (EngineSearcher.search_filterbank), the events are gathered as the peak
    lists are, and the return is (peak list, pulses): the SinglePulse list of
    single_pulse.cluster_events over the events of every DM, on every rank."""
    fb, dms, kdm, world, mine, nout = _filterbank_shard(fb_or_fname, dms, kdm, group)
    local = []
    if dms:
        # zero_dm is passed only when set: a searcher without the argument keeps working
        extra = {"zero_dm": True} if zero_dm else {}
        if pulses is not None:
            extra["pulses"] = pulses
        if block_mask is not None:    # as zero_dm: only when set
            extra["block_mask"] = block_mask
        if inject is not None:
            extra["inject"] = inject
        local = searcher.search_filterbank(fb, [dms[i] for i in mine], mask=mask, nout=nout, kdm=kdm, **extra)
        if pulses is not None:
            local = local[0]
    peaks = _gather_per_dm(mine, local, group, world)
    if pulses is None:
        return peaks
    from . import single_pulse
    events = np.empty(0, dtype=single_pulse.EVENT_DTYPE)
    if mine:
        events = searcher.pulse_events.copy()
        events["series"] = np.asarray(mine, dtype=np.int32)[events["series"]]
    if world > 1:
        import torch.distributed as dist
        gathered = [None] * world
        dist.all_gather_object(gathered, events, group=group)
        events = np.concatenate(gathered)
    events = events[np.lexsort((events["sample"], events["series"]))]
    widths = single_pulse._default_widths(pulses.get("widths"), nout) if dms else None
    return peaks, single_pulse.cluster_events(events, dms, fb.tsamp, time_radius=pulses.get("time_radius"),
                                              dm_gap=pulses.get("dm_gap", 1), widths=widths)


def search_filterbank_accel(fb_or_fname, dms, accels, searcher, group=None, mask=None, kdm=None, zero_dm=False,
                            block_mask=None, inject=None):
    """search_filterbank with an acceleration axis: each rank dedisperses its
    round-robin share of `dms` from the one file, searches every series at
    every trial acceleration of `accels` (m/s^2;
    searcher.search_filterbank_accel, an EngineSearcher), and the tagged peak
    lists are gathered once.  Returns the full list of acceleration.AccelPeak
    on every rank, in the order of `dms`, then of `accels`, then range order.
    Every rank cuts its series to the length the whole DM list leaves, so the
    result does not depend on the sharding -- the stretch is defined on that
    common length.  fb_or_fname, mask, kdm, zero_dm, block_mask and inject as for
    search_filterbank; the single-pulse search is not combined with it."""
    from .acceleration import AccelPeak
    fb, dms, kdm, world, mine, nout = _filterbank_shard(fb_or_fname, dms, kdm, group)
    accels = [float(a) for a in accels]
    local = []
    if dms:
        extra = {} if inject is None else {"inject": inject}    # only when set
        local = searcher.search_filterbank_accel(fb, [dms[i] for i in mine], accels, mask=mask, nout=nout, kdm=kdm,
                                                 zero_dm=zero_dm, block_mask=block_mask, **extra)
    return _gather_per_dm(mine, local, group, world, make=AccelPeak)


def search_filterbank_plan(fb_or_fname, plan, searcher, group=None, mask=None, kdm=None, zero_dm=False,
                           block_mask=None, budget_bytes=None, inject=None):
    """search_filterbank over a dedispersion.DMPlan (dedispersion.dm_plan):
    each rank takes the round-robin share of every step of the plan
    (plan.shard), dedisperses it from the one file with every step decimated
    in time by its factor, and searches each step at its own sampling time
    (searcher.search_filterbank_plan, an EngineSearcher); one gather of the
    tagged peak lists.  Returns the full peak list on every rank, in plan
    order (then range order within a DM): the search_trials contract.  A
    shard keeps the plan's dm_cover, so every rank's series cover the stretch
    of the observation the whole plan leaves and the result does not depend on
    the sharding.  fb_or_fname, mask, kdm, zero_dm, block_mask and inject as for
    search_filterbank; budget_bytes is each rank's device memory for the
    series of one slice of its share (EngineSearcher.search_filterbank_plan).

    Out of scope: pulses= and the acceleration axis with a plan (their events
    and stretches assume one sampling time), and bands= with decimation;
    build_candidates_filterbank folds peaks found on a decimated trial at the
    file's resolution, which works since periods are in seconds."""
    from .reading import Filterbank, open_filterbank
    fb = fb_or_fname if isinstance(fb_or_fname, Filterbank) else open_filterbank(fb_or_fname)
    rank, world = _rank_world(group)
    mine = plan.shard_indices(rank, world)
    local = []
    if mine:
        # set arguments only: a searcher without them keeps working
        extra = {"zero_dm": True} if zero_dm else {}
        if block_mask is not None:
            extra["block_mask"] = block_mask
        if budget_bytes is not None:
            extra["budget_bytes"] = budget_bytes
        if inject is not None:
            extra["inject"] = inject
        local = searcher.search_filterbank_plan(fb, plan.shard(rank, world), mask=mask, kdm=kdm, **extra)
    return _gather_per_dm(mine, local, group, world)
