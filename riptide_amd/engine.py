"""Device-resident, batched hot path (the part bench.py and the multi-GPU
dispatcher drive).  Buffers are torch tensors on the ROCm device; all compute
is the engine's HIP kernels (rt_plan_* / rt_periodogram_device /
rt_deredden_normalise_device in include/riptide_amd.h).
"""
import ctypes
import typing

import numpy as np

from . import _lib
from ._args import (batch_rows, check_workspace, checked_out, checked_workspace, resolve_device, stream_on,
                    stream_scope)
from .ffautils import generate_width_trials

_L = _lib.load()
_check = _lib.check


def _size(fn, *args):
    """The value a size query of the C API writes to its size_t out-parameter."""
    b = ctypes.c_size_t()
    _check(fn(*args, ctypes.byref(b)))
    return b.value


def _stream_handle(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


# rt_ladder_rung (include/riptide_amd.h)
LADDER_RUNG_DTYPE = np.dtype([("f", np.float64), ("n", np.uint64), ("leaf_off", np.uint64), ("fused", np.uint32),
                              ("reserved", np.uint32)])


def ladder_layout(size, tsamp, period_min, period_max, bins_min, bins_max):
    """Where a plan of these search parameters puts its downsampling ladder
    (rt_ladder_layout; host only, no device): a dict of
      rungs        one record per rung that feeds a transform (LADDER_RUNG_DTYPE):
                   factor f, length n, float offset leaf_off of the rung in a
                   trial's leaf buffer, fused = 1 if the fused kernel writes it
      leaf_floats  floats of one trial's leaf buffer (trial b's starts b *
                   leaf_floats floats into the workspace)
      mode         0 per-rung kernel, 1 fused, 2 both (rt_ladder_check)
      margin       samples the fused kernel stages past each span (0: not run)
    RIPTIDE_AMD_PER_RUNG_LADDER, which only plan creation honours, is not
    reflected: such a plan has the same offsets and mode 0."""
    args = (int(size), float(tsamp), float(period_min), float(period_max), int(bins_min), int(bins_max))
    count, leaf = ctypes.c_uint64(), ctypes.c_uint64()
    mode, margin = ctypes.c_int(), ctypes.c_uint32()
    _check(_L.rt_ladder_layout(*args, None, 0, ctypes.byref(count), None, None, None))
    rungs = np.zeros(count.value, dtype=LADDER_RUNG_DTYPE)
    _check(_L.rt_ladder_layout(*args, _lib.ptr(rungs), rungs.size, ctypes.byref(count), ctypes.byref(leaf),
                               ctypes.byref(mode), ctypes.byref(margin)))
    return {"rungs": rungs, "leaf_floats": leaf.value, "mode": mode.value, "margin": margin.value}


# rt_schedule_item (include/riptide_amd.h)
SCHEDULE_ITEM_DTYPE = np.dtype([(k, np.uint32) for k in
                                ("launch", "pass", "slots", "snr_kind", "xform", "rung", "bins", "node_start",
                                 "node_size", "s0", "s1", "levels", "src_leaves", "tile")])


def schedule_items(size, tsamp, period_min, period_max, bins_min, bins_max, num_widths=0):
    """The work units of the cone schedule of these search parameters in
    dispatch order, launch after launch (rt_schedule_items; host only, no
    device): one SCHEDULE_ITEM_DTYPE record per unit."""
    args = (int(size), float(tsamp), int(num_widths), float(period_min), float(period_max), int(bins_min),
            int(bins_max))
    count = ctypes.c_uint64()
    _check(_L.rt_schedule_items(*args, None, 0, ctypes.byref(count)))
    items = np.zeros(count.value, dtype=SCHEDULE_ITEM_DTYPE)
    _check(_L.rt_schedule_items(*args, _lib.ptr(items), items.size, ctypes.byref(count)))
    return items


class PeriodogramPlan:
    """Compiled periodogram plan for series of `size` samples: downsampling
    ladder, trial grid and the cone-kernel pass schedule (host-built once,
    uploaded to the current device)."""

    def __init__(self, size, tsamp, widths, period_min, period_max, bins_min, bins_max, device=None):
        import torch
        dev = resolve_device(device)
        _check(_L.rt_set_device(dev.index))
        self.device = dev
        self.size, self.tsamp = int(size), float(tsamp)
        self.widths = np.ascontiguousarray(widths, dtype=np.uint64)
        self.period_min, self.period_max = float(period_min), float(period_max)
        self.bins_min, self.bins_max = int(bins_min), int(bins_max)
        h = ctypes.c_void_p()
        with torch.cuda.device(dev):
            _check(_L.rt_plan_create(self.size, self.tsamp, _lib.ptr(self.widths), self.widths.size,
                                     self.period_min, self.period_max, self.bins_min, self.bins_max,
                                     ctypes.byref(h)))
        self._h = h
        L, W = ctypes.c_size_t(), ctypes.c_size_t()
        _check(_L.rt_plan_shape(h, ctypes.byref(L), ctypes.byref(W)))
        self.length, self.num_widths = L.value, W.value
        self._grid = None

    @classmethod
    def for_search(cls, size, tsamp, period_min, period_max, bins_min=240, bins_max=260, ducy_max=0.2,
                   wtsp=1.5, device=None):
        widths = generate_width_trials(bins_min, ducy_max=ducy_max, wtsp=wtsp)
        return cls(size, tsamp, widths, period_min, period_max, bins_min, bins_max, device=device)

    def grid(self):
        """(periods f64[L], foldbins u32[L]) -- bit-exact with the reference."""
        if self._grid is None:
            periods = np.empty(self.length, dtype=np.float64)
            foldbins = np.empty(self.length, dtype=np.uint32)
            _check(_L.rt_plan_grid(self._h, _lib.ptr(periods), _lib.ptr(foldbins)))
            self._grid = (periods, foldbins)
        return self._grid

    def workspace_bytes(self, batch):
        return _size(_L.rt_plan_workspace_bytes, self._h, int(batch))

    def ladder_layout(self):
        """ladder_layout() of this plan's own search parameters."""
        return ladder_layout(self.size, self.tsamp, self.period_min, self.period_max, self.bins_min, self.bins_max)

    def stats(self):
        u = [ctypes.c_uint64() for _ in range(4)]
        d = [ctypes.c_double() for _ in range(2)]
        _check(_L.rt_plan_stats(self._h, *(ctypes.byref(x) for x in u[:3]), ctypes.byref(d[0]),
                                ctypes.byref(d[1]), ctypes.byref(u[3])))
        return {"transforms": u[0].value, "items": u[1].value, "launches": u[2].value,
                "alg_bytes": d[0].value, "moved_bytes": d[1].value, "cells": u[3].value}

    def run(self, data, out=None, workspace=None, stream=None, check=False):
        """S/N of a batch of series: data float32 [B, size] (or [size]) on the
        device -> float32 [B, L, W].  Stream-ordered; no host synchronisation
        unless `check` (then the plan's device error flag is read: see
        check()).  Allocations happen on `stream` (default: the current one)."""
        import torch
        squeeze = data.dim() == 1
        if squeeze:
            data = data.unsqueeze(0)
        B = self._rows(data)
        with stream_scope(self.device, stream) as (s, handle):
            out = checked_out(out, (B, self.length, self.num_widths), torch.float32, self.device,
                              f"out must be a contiguous float32 [{B}, {self.length}, {self.num_widths}] "
                              "tensor on the plan's device")
            workspace = checked_workspace(workspace, self.workspace_bytes(B), self.device, "plan")
            _check(_L.rt_periodogram_device(self._h, _lib.ptr(data), B, data.stride(0), _lib.ptr(out),
                                            self.length * self.num_widths, _lib.ptr(workspace), workspace.numel(),
                                            handle))
        if check:
            self.check(s)
        return out[0] if squeeze else out

    def _rows(self, data):
        """B of a batch argument of run() or ladder(), checked."""
        import torch
        if data.dim() != 2 or data.dtype != torch.float32 or data.device != self.device or data.shape[1] != self.size:
            raise ValueError("data must be float32 [B, size] on the plan's device")
        if data.stride(1) != 1:
            raise ValueError("data rows must be contiguous")
        return data.shape[0]

    def ladder(self, data, workspace, stream=None):
        """First half of run(): the downsampling ladder of data float32 [B, size]
        into `workspace`'s leaf buffer (rt_periodogram_ladder_device).  With
        passes() on another stream, batch k + 1's ladder overlaps batch k's
        FFA passes; the caller orders the two halves of one batch (an event)
        and keeps a workspace per batch in flight."""
        B = self._rows(data)
        check_workspace(workspace, self.workspace_bytes(B), self.device, "plan")
        _check(_L.rt_periodogram_ladder_device(self._h, _lib.ptr(data), B, data.stride(0), _lib.ptr(workspace),
                                               workspace.numel(), _stream_handle(stream_on(self.device, stream))))

    def passes(self, out, workspace, stream=None):
        """Second half of run(): FFA passes + fused S/N of the batch whose
        ladder filled `workspace`, into out float32 [B, L, W]."""
        import torch
        B, L, W = out.shape[0], self.length, self.num_widths
        checked_out(out, (B, L, W), torch.float32, self.device,
                    f"out must be a contiguous float32 [B, {L}, {W}] tensor on the plan's device")
        check_workspace(workspace, self.workspace_bytes(B), self.device, "plan")
        _check(_L.rt_periodogram_passes_device(self._h, B, _lib.ptr(out), self.length * self.num_widths,
                                               _lib.ptr(workspace), workspace.numel(),
                                               _stream_handle(stream_on(self.device, stream))))
        return out

    def check(self, stream=None):
        """Raise EngineError if any cone work unit of the runs since the last
        check broke its LDS / register budget (its S/N rows were left
        unwritten).  Synchronises `stream` (default: the current stream)."""
        _check(_L.rt_plan_check(self._h, _stream_handle(stream)))

    def __del__(self, _destroy=_L.rt_plan_destroy):
        # the default argument keeps the function alive through interpreter
        # shutdown, when module globals may already be cleared
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            _destroy(h)
            self._h = None


def deredden_workspace_bytes(size, width_samples, min_points, batch):
    return _size(_L.rt_deredden_workspace_bytes, int(size), int(width_samples), int(min_points), int(batch))


# rt_dered_forms and its RT_* values (include/riptide_amd.h)
DERED_FORMS_DTYPE = np.dtype([("scrunch_factor", np.uint64), ("n_lo", np.uint64), ("rmed_width", np.uint64),
                              ("scrunch", np.uint32), ("scrunch_chunks", np.uint32), ("rmed", np.uint32),
                              ("subtract", np.uint32), ("fused", np.uint32), ("norm_partial", np.uint32),
                              ("norm_passes", np.uint32), ("norm_apply", np.uint32)])
SCRUNCH_STAGED_VEC, SCRUNCH_STAGED, SCRUNCH_GENERAL = 1, 2, 3
RMED_SMALL, RMED_LARGE = 1, 2
SUBTRACT_PER_SAMPLE, SUBTRACT_SLOPE1, SUBTRACT_SLOPE4 = 1, 2, 3
NORM_SCALAR, NORM_VEC = 1, 2


def deredden_forms(size, width_samples, min_points=101, deredden=True, normalise=True, in_align=0, out_align=0,
                   in_stride=None, out_stride=None):
    """The kernel form each stage of deredden_normalise takes for rows of
    `size` samples at device addresses in_align / out_align bytes past a
    16-byte boundary, in_stride / out_stride floats apart (default: size), as
    a dict of DERED_FORMS_DTYPE's fields (rt_deredden_forms; host only, no
    device).  A stage that does not run is 0; the environment switches are not
    reflected."""
    rec = np.zeros(1, dtype=DERED_FORMS_DTYPE)
    _check(_L.rt_deredden_forms(int(size), int(width_samples), int(min_points), int(bool(deredden)),
                                int(bool(normalise)), int(in_align), int(out_align),
                                int(size if in_stride is None else in_stride),
                                int(size if out_stride is None else out_stride), _lib.ptr(rec)))
    return {k: int(rec[k][0]) for k in DERED_FORMS_DTYPE.names}


def deredden_normalise(data, width_samples, min_points=101, deredden=True, normalise=True, out=None,
                       workspace=None, stream=None):
    """TimeSeries.deredden(...).normalise() for a batch [B, N] of device series."""
    import torch
    data, B, N, squeeze = batch_rows(data)
    dev = data.device
    with stream_scope(dev, stream) as (_, handle):
        out = checked_out(out, (B, N), torch.float32, dev,
                          "out must be float32 [B, N] rows with unit stride on the data's device",
                          lambda o: (o.dim() != 2 or tuple(o.shape) != (B, N) or o.dtype != torch.float32
                                     or o.device != dev or o.stride(1) != 1))
        workspace = checked_workspace(workspace, deredden_workspace_bytes(N, width_samples, min_points, B), dev, "data")
        _check(_L.rt_deredden_normalise_device(_lib.ptr(data), N, B, data.stride(0), int(width_samples),
                                               int(min_points), int(bool(deredden)), int(bool(normalise)),
                                               _lib.ptr(out), out.stride(0), _lib.ptr(workspace), workspace.numel(),
                                               handle))
    return out[0] if squeeze else out


def fold_device(data, tsamp, specs, stream=None):
    """folding.fold for a batch of candidates of device-resident series
    (rt_fold_device): data float32 [N] or [B, N], specs a list of
    (series, period, bins, subints).  Returns one device tensor per spec,
    (bins,) or (rows, bins), all views of one output allocation, bit-identical
    to folding.fold of the same series.  Stream-ordered, no host
    synchronisation.  Raises folding.fold's ValueErrors."""
    import torch
    from .folding import pack_fold_specs
    data, B, N, _ = batch_rows(data)
    specs = list(specs)
    if not specs:
        return []
    for series, _, bins, _ in specs:
        if not 0 <= int(series) < B:
            raise ValueError(f"series index {series} outside the {B} rows of data")
        if int(bins) < 2:
            raise ValueError("the device fold needs bins >= 2")
    table, shapes, total = pack_fold_specs(N, N * float(tsamp), float(tsamp), specs)
    need = _size(_L.rt_fold_workspace_bytes, N, _lib.ptr(table), len(specs))
    with stream_scope(data.device, stream) as (_, handle):
        out = torch.empty(total, dtype=torch.float32, device=data.device)
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=data.device)
        _check(_L.rt_fold_device(_lib.ptr(data), N, data.stride(0), B, _lib.ptr(table), len(specs), _lib.ptr(out),
                                 total, _lib.ptr(workspace), workspace.numel(), handle))
    results = []
    for k, shape in enumerate(shapes):
        o = int(table["out_off"][k])
        results.append(out[o:o + int(np.prod(shape))].view(*shape))
    return results


def refine_device(cubes, shifts, widths, table, profiles=False, stream=None):
    """refine.refine_many for arrays that stay on the device
    (rt_refine_device): cubes float32, shifts int32 and widths int32 (values
    below 2^31, read as uint32) are flat device tensors, packed as
    refine.pack_refine packs them; table is its host REFINE_SPEC array.
    Returns (snr, prof): flat float32 device tensors holding each candidate's
    [K, J, W] and [K, J, N] at its snr_off / prof_off (prof is None without
    profiles=True).  Stream-ordered, no host synchronisation.

    The device tables are not validated, and need not be: a shift v is used
    as (v mod 2^32) mod bins and a width is clamped to [1, bins - 1].  Every
    offset of `table` must lie inside the tensors: that is checked here."""
    import torch
    from .refine import REFINE_SPEC
    table = np.ascontiguousarray(table, dtype=REFINE_SPEC)
    for t, dt, name in ((cubes, torch.float32, "cubes"), (shifts, torch.int32, "shifts"), (widths, torch.int32, "widths")):
        if t.dim() != 1 or t.dtype != dt or t.device.type != "cuda" or not t.is_contiguous():
            raise ValueError(f"{name} must be a flat contiguous {dt} device tensor")
    if not table.size:
        return torch.empty(0, dtype=torch.float32, device=cubes.device), None
    u = {k: table[k].astype(np.uint64) for k in table.dtype.names if k not in ("stdnoise", "reserved")}
    if (int((u["cube_off"] + u["bands"] * u["subints"] * u["bins"]).max()) > cubes.numel()
            or int((u["dshift_off"] + u["ndm"] * u["bands"]).max()) > shifts.numel()
            or int((u["pshift_off"] + u["nper"] * u["subints"]).max()) > shifts.numel()
            or int((u["width_off"] + u["nw"]).max()) > widths.numel()):
        raise ValueError("refine: a spec's arrays exceed the device tensors")
    nsnr = int((u["snr_off"] + u["ndm"] * u["nper"] * u["nw"]).max())
    nprof = int((u["prof_off"] + u["ndm"] * u["nper"] * u["bins"]).max())
    need = _size(_L.rt_refine_workspace_bytes, _lib.ptr(table), table.size)
    with stream_scope(cubes.device, stream) as (_, handle):
        snr = torch.empty(nsnr, dtype=torch.float32, device=cubes.device)
        prof = torch.empty(nprof, dtype=torch.float32, device=cubes.device) if profiles else None
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=cubes.device)
        _check(_L.rt_refine_device(_lib.ptr(cubes), _lib.ptr(shifts), _lib.ptr(widths), _lib.ptr(table), table.size,
                                   _lib.ptr(snr), _lib.ptr(prof) if profiles else None, _lib.ptr(workspace),
                                   workspace.numel(), handle))
    return snr, prof


def _pulse_limits():
    tile, wmax = ctypes.c_size_t(), ctypes.c_size_t()
    _check(_L.rt_single_pulse_limits(ctypes.byref(tile), ctypes.byref(wmax)))
    return tile.value, wmax.value


# the single-pulse kernel's tile length in samples, and RT_PULSE_MAX_WIDTH
# (the largest width and radius; include/riptide_amd.h)
PULSE_TILE, PULSE_MAX_WIDTH = _pulse_limits()
# rt_pulse_event (include/riptide_amd.h)
PULSE_EVENT_DTYPE = np.dtype([("series", np.int32), ("sample", np.int32), ("iwidth", np.int32), ("snr", np.float32)])


def pulse_plan(wmax, radius):
    """(chunk, chunk_segs, lds_bytes) of the single-pulse tile kernel for a
    largest width and a radius (rt_single_pulse_plan; no device call): the
    tile's T + 2 * radius outputs are worked through `chunk` at a time."""
    if int(wmax) < 0 or int(radius) < 0:
        raise ValueError("single pulse: wmax and radius must be >= 0")
    chunk, segs, lds = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    _check(_L.rt_single_pulse_plan(int(wmax), int(radius), ctypes.byref(chunk), ctypes.byref(segs), ctypes.byref(lds)))
    return chunk.value, segs.value, lds.value


class PulseEvents(typing.NamedTuple):
    """The events of single_pulse_device as columns (device tensors of one
    length), sorted by (series, sample)."""
    series: typing.Any      # int32: row of the batch
    sample: typing.Any      # int32
    iwidth: typing.Any      # int32: index into the widths
    snr: typing.Any         # float32


def single_pulse_device(data, widths, threshold, radius=None, dense=False, max_events=1 << 20, stream=None,
                        capacity=None):
    """Single-pulse search of a batch of normalised device series
    (rt_single_pulse_device; the specification: single_pulse.single_pulse_host,
    bit for bit): data float32 [N] or [B, N] with unit sample stride (rows may
    be any distance >= N apart: slices of a wider tensor are read in place),
    widths ascending int samples, radius the local-maximum radius in samples
    (default: the largest width).  Returns PulseEvents, and with dense=True
    (events, best, kbest): float32 and int32 [B, N].

    The events are counted on the device; `capacity` is the room of the first
    attempt (default 4096, at most max_events).  When more are found the call
    is repeated once with room for all of them, and ValueError is raised when
    there are more than max_events.  The count is read back, so the call
    waits for the stream; rt_single_pulse_device itself does not."""
    import torch
    data, B, N, _ = batch_rows(data)
    if B > 1 and data.stride(0) < N:
        raise ValueError("data rows must not overlap")
    w = np.ascontiguousarray(widths, dtype=np.int32).ravel()
    if not w.size:
        raise ValueError("single pulse: no trial widths")
    radius = int(w.max() if radius is None else radius)
    if radius < 0:
        raise ValueError("radius must be >= 0")
    max_events = int(max_events)
    if max_events < 0:
        raise ValueError("max_events must be >= 0")
    cap = min(max_events, 4096 if capacity is None else int(capacity))
    if cap < 0:
        raise ValueError("capacity must be >= 0")
    ldx = data.stride(0) if B > 1 else max(N, 1)
    dev = data.device
    with stream_scope(dev, stream) as (_, handle):
        best = torch.empty((B, N), dtype=torch.float32, device=dev) if dense else None
        kbest = torch.empty((B, N), dtype=torch.int32, device=dev) if dense else None
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        while True:
            ev = torch.empty((cap, 4), dtype=torch.int32, device=dev)
            need = _size(_L.rt_single_pulse_workspace_bytes, B, N, w.size, cap)
            workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            _check(_L.rt_single_pulse_device(_lib.ptr(data), B, N, ldx, _lib.ptr(w), w.size, float(threshold), radius,
                                             _lib.ptr(ev) if cap else None, cap, _lib.ptr(count),
                                             _lib.ptr(best) if dense else None, _lib.ptr(kbest) if dense else None,
                                             _lib.ptr(workspace), workspace.numel(), handle))
            found = int(count.item())
            if found <= cap:
                break
            if found > max_events:
                raise ValueError(f"single pulse: {found} events at threshold {float(threshold):g} exceed max_events = "
                                 f"{max_events}; raise the threshold")
            cap = found
        ev = ev[:found]
        events = PulseEvents(ev[:, 0], ev[:, 1], ev[:, 2], ev[:, 3].view(torch.float32))
    return (events, best, kbest) if dense else events


def resample_device(data, factors, src=None, out=None, stream=None):
    """Time-domain resampling of a batch of device series for the acceleration
    search (rt_resample_device; the specification: acceleration.resample_host,
    bit for bit): data float32 [N] or [B, N] with unit sample stride (rows may
    be any distance >= N apart: slices of a wider tensor are read in place),
    factors float64 values on the host (acceleration.accel_factor), src None
    -- every row with every factor, row-major [B, len(factors)] -- or one
    source row per factor.  Returns out, float32 [R, N] on the data's device
    (allocated when None; rows with unit sample stride, any distance >= N
    apart, not overlapping data).  Stream-ordered, no host synchronisation, no
    workspace.  ValueError, nothing launched, for N above 2^27, R above 65535,
    a src outside [0, B), a factor that is not finite or has |f| * N >= 1."""
    import torch
    from .acceleration import resample_rows
    data, B, N, _ = batch_rows(data)
    if B > 1 and data.stride(0) < N:
        raise ValueError("resample: input row stride below the series length")
    rows, f = resample_rows(B, factors, src)
    R = rows.size
    dev = data.device
    with stream_scope(dev, stream) as (_, handle):
        out = checked_out(out, (R, N), torch.float32, dev,
                          f"out must be float32 [{R}, {N}] rows with unit stride on the data's device",
                          lambda o: (o.dim() != 2 or tuple(o.shape) != (R, N) or o.dtype != torch.float32
                                     or o.device != dev or o.stride(1) != 1))
        if R > 1 and out.stride(0) < N:
            raise ValueError("resample: output row stride below the series length")
        _check(_L.rt_resample_device(_lib.ptr(data), B, N, data.stride(0) if B > 1 else max(N, 1), _lib.ptr(rows),
                                     _lib.ptr(f), R, _lib.ptr(out), out.stride(0) if R > 1 else max(N, 1), handle))
    return out


# RT_DEDISP_* sample type codes (include/riptide_amd.h); 'u1', 'u2', 'u4' and
# 'u16' are the packed types: the block is then uint8 rows of nchans * nbits / 8
# bytes (reading.unpack_samples has the format)
DEDISP_DTYPES = {"uint8": 0, "int8": 1, "float32": 2, "u1": 0x101, "u2": 0x102, "u4": 0x104, "u16": 0x110}
DEDISP_PACKED_NBITS = (1, 2, 4, 16)    # the nbits of the packed keys; every other key is a numpy dtype's name
DEDISP_ZERO_DM = 1    # RT_DEDISP_ZERO_DM, the one flag bit
# (dedispersion.py and rfi.py take the codes and the flag from here)


def _dedisp_name(dtype, nbits):
    """The key of DEDISP_DTYPES for a dtype name, or for packed `nbits`."""
    name = str(dtype) if nbits is None else f"u{int(nbits)}"
    if name not in DEDISP_DTYPES or (nbits is not None and int(nbits) not in DEDISP_PACKED_NBITS):
        raise ValueError("the sample type must be uint8, int8, float32, or packed with nbits 1, 2, 4 or 16")
    return name


def checked_bands(bands, nchans):
    """bands as a contiguous uint32 [nbands, 2] array of channel ranges
    [lo, hi) with lo <= hi <= nchans; ValueError otherwise."""
    b = np.asarray(bands)
    if b.ndim != 2 or b.shape[1] != 2 or b.dtype.kind not in "iu":
        raise ValueError("bands must be an integer array [nbands, 2] of channel ranges [lo, hi)")
    if b.size and (b.min() < 0 or np.any(b[:, 0] > b[:, 1]) or b[:, 1].max() > nchans):
        raise ValueError(f"every band must be a channel range lo <= hi <= {nchans}")
    return np.ascontiguousarray(b, dtype=np.uint32)


def dedisperse_workspace_bytes(dtype, nsamp_blk, nchans, zero_dm=False, nbits=None):
    """Device workspace bytes of dedisperse_device for a block of this shape;
    dtype is 'uint8', 'int8', 'float32' or a packed type name ('u1', 'u2',
    'u4', 'u16'; or pass nbits, dtype is then ignored).  1/2/4-bit data takes
    the 8-bit size and 16-bit data the float32 size.  With zero_dm every dtype
    takes float32 rows, plus nsamp_blk floats for the mean series."""
    return _size(_L.rt_dedisperse_workspace_bytes_opt, DEDISP_DTYPES[_dedisp_name(dtype, nbits)], int(nsamp_blk),
                 int(nchans), DEDISP_ZERO_DM if zero_dm else 0)


def dedisperse_span_plan(esize, lo, hi):
    """(ndw, staged) of the dedispersion sum kernel for one channel of one
    tile of 16 DMs x 256 outputs (rt_dedisperse_span_plan; no device call):
    esize is 1 for 8-bit rows (uint8, int8, 1/2/4-bit data) and 4 for float
    rows (float32, 16-bit data, everything under zero_dm); lo and hi are the
    smallest and largest delay, clamped to [0, max_delay], of the tile's DMs
    in that channel.  ndw is the dwords the channel's span takes; staged says
    whether they go through LDS (8-bit rows: hi - (lo & ~3) <= 800; float
    rows: hi - lo <= 264) or the channel is read from its workspace row
    directly.  ValueError for another esize, lo < 0, lo > hi or hi >= 2^31."""
    ndw, staged = ctypes.c_size_t(), ctypes.c_int()
    _check(_L.rt_dedisperse_span_plan(int(esize), int(lo), int(hi), ctypes.byref(ndw), ctypes.byref(staged)))
    return ndw.value, bool(staged.value)


def _dedisp_block(block, nbits=None):
    """(dtype name, nsamp_blk, nchans) of a block argument, validated.  With
    nbits the block is packed rows, uint8 [nsamp_blk, row_bytes] (any byte
    alignment), and nchans = row_bytes * 8 / nbits."""
    if block.dim() != 2 or block.device.type != "cuda" or not block.is_contiguous():
        raise ValueError("block must be a contiguous [nsamp_blk, nchans] device tensor")
    name = str(block.dtype).replace("torch.", "")
    if nbits is not None:
        if name != "uint8":
            raise ValueError("a packed block must be uint8 [nsamp_blk, row_bytes]")
        name = _dedisp_name(None, nbits)
        if block.shape[1] * 8 % int(nbits):
            raise ValueError(f"rows of {block.shape[1]} bytes are not a whole number of {int(nbits)}-bit channels")
        return name, block.shape[0], block.shape[1] * 8 // int(nbits)
    if name not in DEDISP_DTYPES:
        raise ValueError("block must be uint8, int8 or float32")
    return name, block.shape[0], block.shape[1]


def _check_device_mask(mask, block, nchans):
    import torch
    if mask is not None and (mask.dtype != torch.uint8 or mask.device != block.device or not mask.is_contiguous()
                             or tuple(mask.shape) != (nchans,)):
        raise ValueError("mask must be a contiguous uint8 [nchans] tensor on the block's device")


# dtype names a block mask's fill may have, by sample type name: the sample's
# own type (include/riptide_amd.h, rt_block_mask); 1/2/4-bit data takes one
# unpacked value per byte, 16-bit data uint16 (or int16 holding the same bits)
_FILL_DTYPES = {"uint8": ("uint8",), "int8": ("int8",), "float32": ("float32",), "u1": ("uint8",), "u2": ("uint8",),
                "u4": ("uint8",), "u16": ("uint16", "int16")}


class DeviceBlockMask:
    """A block mask in device memory, the block_mask= argument of
    dedisperse_device, dedisperse_bands_device and zero_dm_mean_device
    (rt_block_mask in include/riptide_amd.h): `cells` uint8 [nblocks, nchans],
    non-zero = the channel is flagged during block b, the absolute samples
    [b * block_len, (b + 1) * block_len); `fill` [nchans] in the sample's own
    type (uint8 for uint8 and 1/2/4-bit data, int8, float32, uint16); the int
    `block_len`.  A holder: the calls validate it against their block."""

    def __init__(self, cells, fill, block_len):
        self.cells, self.fill, self.block_len = cells, fill, int(block_len)

    def __repr__(self):
        return f"DeviceBlockMask(cells={tuple(self.cells.shape)}, block_len={self.block_len})"


def _block_mask_struct(block_mask, t_origin, block, name, nchans):
    """The rt_block_mask of a block_mask= argument, validated the way
    _check_device_mask validates a channel mask; None for None.  Whether the
    rows lie inside the mask is the entry point's check."""
    import torch
    if block_mask is None:
        return None
    cells, fill, block_len = block_mask.cells, block_mask.fill, int(block_mask.block_len)
    if block_len < 1:
        raise ValueError("block_mask: block_len must be at least 1")
    if not 0 <= int(t_origin) < 1 << 64:
        raise ValueError("t_origin must be in [0, 2^64)")
    if (not torch.is_tensor(cells) or cells.dtype != torch.uint8 or cells.device != block.device or cells.dim() != 2
            or not cells.is_contiguous() or cells.shape[1] != nchans):
        raise ValueError(f"block_mask.cells must be a contiguous uint8 [nblocks, {nchans}] tensor on the block's "
                         "device")
    wanted = _FILL_DTYPES[name]
    if (not torch.is_tensor(fill) or str(fill.dtype).replace("torch.", "") not in wanted
            or fill.device != block.device or not fill.is_contiguous() or tuple(fill.shape) != (nchans,)):
        raise ValueError(f"block_mask.fill must be a contiguous {wanted[0]} [{nchans}] tensor on the block's device: "
                         "one value per channel in the sample's own type")
    return _lib.BlockMaskStruct(cells.data_ptr(), cells.shape[0], block_len, int(t_origin), fill.data_ptr())


def zero_dm_mean_device(block, mask=None, out=None, stream=None, nbits=None, block_mask=None, t_origin=0):
    """The zero-DM time series of one resident block (rt_zero_dm_mean_device,
    the row-mean kernel alone): float32 [nsamp_blk], every time sample's mean
    over the unmasked channels -- the sum exact for 8-bit data, in float64 for
    float32 data, divided in float64 and rounded to float32 once; all zero
    when every channel is masked.  block, mask, nbits, block_mask and t_origin
    as for dedisperse_device (packed sums are exact integers too): with a block
    mask the series is that of x', the bits of the plain call on x'.
    Stream-ordered, no host synchronisation."""
    import torch
    name, nsamp_blk, nchans = _dedisp_block(block, nbits)
    _check_device_mask(mask, block, nchans)
    bm = _block_mask_struct(block_mask, t_origin, block, name, nchans)
    with stream_scope(block.device, stream) as (_, handle):
        out = checked_out(out, (nsamp_blk,), torch.float32, block.device,
                          f"out must be a contiguous float32 [{nsamp_blk}] tensor on the block's device")
        if nsamp_blk:
            args = (_lib.ptr(block), DEDISP_DTYPES[name], nsamp_blk, nchans, None if mask is None else _lib.ptr(mask),
                    _lib.ptr(out), handle)
            if bm is None:
                _check(_L.rt_zero_dm_mean_device(*args))
            else:
                _check(_L.rt_zero_dm_mean_device_cells(*args, ctypes.byref(bm)))
    return out


def block_stats_workspace_bytes(nsamp_blk, nchans, block_len):
    """Device workspace bytes of block_stats_device for a block of this shape
    (none for block_len <= 2048)."""
    return _size(_L.rt_block_stats_workspace_bytes, int(nsamp_blk), int(nchans), int(block_len))


def block_stats_device(block, block_len, out=None, workspace=None, stream=None, nbits=None):
    """Per (block of block_len time samples, channel) sum and sum of squares of
    one resident block (rt_block_stats_device): float64 [nblk, 2, nchans] on
    the block's device, nblk = ceil(nsamp_blk / block_len), blocks counted from
    the block's row 0, the last one possibly partial; written, not added.
    Integer samples give exact integers; float32 sums follow the fixed order of
    rt_block_stats_host and equal it bit for bit.  No atomics: the same bits
    every time.  block and nbits as for dedisperse_device.  Stream-ordered, no
    host synchronisation.  Returns out."""
    import torch
    name, nsamp_blk, nchans = _dedisp_block(block, nbits)
    block_len = int(block_len)
    if block_len < 1:
        raise ValueError("block_stats: block_len must be at least 1")
    nblk = -(-nsamp_blk // block_len)
    with stream_scope(block.device, stream) as (_, handle):
        out = checked_out(out, (nblk, 2, nchans), torch.float64, block.device,
                          f"out must be a contiguous float64 [{nblk}, 2, {nchans}] tensor on the block's device")
        if not nsamp_blk:
            return out
        workspace = checked_workspace(workspace, block_stats_workspace_bytes(nsamp_blk, nchans, block_len),
                                      block.device, "block", floor=16)
        _check(_L.rt_block_stats_device(_lib.ptr(block), DEDISP_DTYPES[name], nsamp_blk, nchans, block_len,
                                        _lib.ptr(out), _lib.ptr(workspace), workspace.numel(), handle))
    return out


def channel_stats_workspace_bytes(nsamp_blk, nchans):
    """Device workspace bytes of channel_stats_device for a block of this shape."""
    return _size(_L.rt_channel_stats_workspace_bytes, int(nsamp_blk), int(nchans))


def channel_stats_device(block, acc, workspace=None, stream=None, nbits=None):
    """Add the per-channel sums of one resident block into acc, float64
    [2, nchans] on the block's device (rt_channel_stats_device): acc[0] += the
    sum over time of block[:, c], acc[1] += the sum of its squares (int8
    samples as signed values).  Partial sums per chunk of time, folded in
    chunk order: no atomics, the same bits every time; 8-bit sums are exact.
    nbits: the block is packed rows, as for dedisperse_device; the sums are
    integers, exact below 2^53.
    Stream-ordered, no host synchronisation.  Returns acc."""
    import torch
    name, nsamp_blk, nchans = _dedisp_block(block, nbits)
    if (acc.dtype != torch.float64 or acc.device != block.device or not acc.is_contiguous()
            or tuple(acc.shape) != (2, nchans)):
        raise ValueError(f"acc must be a contiguous float64 [2, {nchans}] tensor on the block's device")
    with stream_scope(block.device, stream) as (_, handle):
        if not nsamp_blk:
            return acc
        workspace = checked_workspace(workspace, channel_stats_workspace_bytes(nsamp_blk, nchans), block.device,
                                      "block", floor=16)
        _check(_L.rt_channel_stats_device(_lib.ptr(block), DEDISP_DTYPES[name], nsamp_blk, nchans, _lib.ptr(acc),
                                          _lib.ptr(workspace), workspace.numel(), handle))
    return acc


def _dedisperse_device(block, delays, max_delay, bands, mask, out, out_offset, workspace, stream, zero_dm, nbits,
                       block_mask=None, t_origin=0):
    """dedisperse_device (bands None) and dedisperse_bands_device: what they
    share -- block, delays, mask, max_delay, workspace, stream and the block
    mask -- checked once, out by the rule of whichever it is, then the one
    call: without a block mask the entry point it always was, with one
    rt_dedisperse_device_cells."""
    import torch
    name, nsamp_blk, nchans = _dedisp_block(block, nbits)
    bm = _block_mask_struct(block_mask, t_origin, block, name, nchans)
    if (delays.dim() != 2 or delays.dtype != torch.int32 or delays.device != block.device
            or not delays.is_contiguous() or delays.shape[1] != nchans):
        raise ValueError("delays must be a contiguous int32 [ndm, nchans] tensor on the block's device")
    ndm = delays.shape[0]
    _check_device_mask(mask, block, nchans)
    max_delay, out_offset = int(max_delay), int(out_offset)
    nout = nsamp_blk - max_delay
    with stream_scope(block.device, stream) as (_, handle):
        if bands is not None:
            if not torch.is_tensor(bands):
                bands = torch.from_numpy(checked_bands(bands, nchans).view(np.int32)).to(block.device)
            if (bands.dim() != 2 or bands.dtype != torch.int32 or bands.device != block.device
                    or not bands.is_contiguous() or bands.shape[1] != 2):
                raise ValueError("bands must be uint32 [nbands, 2] (as a tensor: contiguous int32 on the block's "
                                 "device)")
            nbands = bands.shape[0]
        # validates the shape before anything is allocated
        need = dedisperse_workspace_bytes(name, nsamp_blk, nchans, zero_dm)
        if not 0 <= max_delay < nsamp_blk:
            raise ValueError(f"max_delay {max_delay} must be in [0, {nsamp_blk}): the block is no longer than the "
                             "largest delay")
        if bands is None:
            out = checked_out(out, (ndm, nout), torch.float32, block.device,
                              f"out must be float32 [{ndm}, >= {out_offset + nout}] rows with unit stride on "
                              "the block's device",
                              lambda o: (o.dim() != 2 or o.dtype != torch.float32 or o.device != block.device
                                         or o.shape[0] != ndm or o.stride(1) != 1 or o.shape[1] < out_offset + nout
                                         or (ndm > 1 and o.stride(0) < o.shape[1])))
        else:
            out = checked_out(out, (ndm, nbands, nout), torch.float32, block.device,
                              f"out must be a contiguous float32 [{ndm}, {nbands}, >= {out_offset + nout}] "
                              "tensor on the block's device",
                              lambda o: (o.dim() != 3 or o.dtype != torch.float32 or o.device != block.device
                                         or tuple(o.shape[:2]) != (ndm, nbands) or not o.is_contiguous()
                                         or o.shape[2] < out_offset + nout))
        workspace = checked_workspace(workspace, need, block.device, "block", floor=16)
        head = (_lib.ptr(block), DEDISP_DTYPES[name], nsamp_blk, nchans, _lib.ptr(delays),
                None if mask is None else _lib.ptr(mask), ndm)
        tail = (out_offset, _lib.ptr(workspace), workspace.numel(), handle, DEDISP_ZERO_DM if zero_dm else 0)
        if bm is not None:
            # the entry point reads "no table, nbands 0" as the plain call: an empty table is refused here,
            # as rt_dedisperse_bands_device refuses it
            if bands is not None and not nbands:
                raise ValueError("dedisperse: nbands must be at least 1")
            table = (None, 0) if bands is None else (_lib.ptr(bands), nbands)
            stride = (out.stride(0) if ndm > 1 else out.shape[1]) if bands is None else out.shape[2]
            _check(_L.rt_dedisperse_device_cells(*head, *table, max_delay, _lib.ptr(out), stride, *tail,
                                                 ctypes.byref(bm)))
        elif bands is None:
            _check(_L.rt_dedisperse_device_opt(*head, max_delay, _lib.ptr(out),
                                               out.stride(0) if ndm > 1 else out.shape[1], *tail))
        else:
            _check(_L.rt_dedisperse_bands_device(*head, _lib.ptr(bands) if nbands else None, nbands, max_delay,
                                                 _lib.ptr(out), out.shape[2], *tail))
    return out


def dedisperse_device(block, delays, max_delay, mask=None, out=None, out_offset=0, workspace=None, stream=None,
                      zero_dm=False, nbits=None, block_mask=None, t_origin=0):
    """Incoherent dedispersion of one resident block (rt_dedisperse_device):
    block uint8 / int8 / float32 [nsamp_blk, nchans] (time-major, contiguous),
    delays int32 [ndm, nchans] and mask (uint8 [nchans], non-zero = skipped, or
    None) on the block's device.  Writes out[d, out_offset + t] = the sum over
    unmasked channels of block[t + delays[d, c], c] for t in [0, nsamp_blk -
    max_delay) and returns out (float32 [ndm, >= out_offset + nsamp_blk -
    max_delay], rows with unit stride; allocated [ndm, nsamp_blk - max_delay]
    when None).  Stream-ordered, no host synchronisation.  8-bit results are
    exact; float32 results are summed in channel order.

    nbits (1, 2, 4 or 16): block is packed rows, uint8 [nsamp_blk, row_bytes]
    with row_bytes = nchans * nbits / 8 and any byte alignment, in the format
    of reading.unpack_samples; nchans is derived from it.  1/2/4-bit data is
    unpacked inside the transpose and summed exactly, as 8-bit data; 16-bit
    data is converted exactly and summed in float32 in channel order (exact up
    to 256 channels).

    zero_dm: the zero-DM filter (RT_DEDISP_ZERO_DM in include/riptide_amd.h).
    Every time sample first loses its mean over the unmasked channels
    (zero_dm_mean_device), and every dtype is then summed in float32 in channel
    order; the workspace is the larger one of dedisperse_workspace_bytes(...,
    zero_dm=True).

    block_mask (a DeviceBlockMask) with t_origin, the absolute sample index of
    the block's row 0: every sample (t, c) with block_mask.cells[(t_origin +
    t) // block_len, c] != 0 is read as block_mask.fill[c], in front of
    everything above -- the result is, bit for bit, that of the same call
    without a block mask on a block holding the replaced samples
    (rfi.apply_block_mask_host).  ValueError, nothing launched, when the rows
    [t_origin, t_origin + nsamp_blk) reach past the nblocks * block_len
    samples the cells cover, or the fill is not of the sample's type.  No
    workspace of its own."""
    return _dedisperse_device(block, delays, max_delay, None, mask, out, out_offset, workspace, stream, zero_dm, nbits,
                              block_mask, t_origin)


def dedisperse_bands_device(block, delays, max_delay, bands, mask=None, out=None, out_offset=0, workspace=None,
                            stream=None, zero_dm=False, nbits=None, block_mask=None, t_origin=0):
    """dedisperse_device for every band of a table at once
    (rt_dedisperse_bands_device): bands is uint32 [nbands, 2] of channel
    ranges [lo, hi) -- a numpy array, or a contiguous int32 tensor on the
    block's device holding the same bits -- and
    out[d, b, out_offset + t] = the sum over the unmasked channels c in
    [lo_b, hi_b) of block[t + delays[d, c], c].  Bands may overlap, be empty
    (a row of zeros, as is a band whose channels are all masked) and come in
    any order; the delays are the plain call's, so the bands stay aligned, and
    the row of the band [0, nchans) equals dedisperse_device's bit for bit.
    With zero_dm the mean is over the unmasked channels of the whole block.
    Returns out, float32 [ndm, nbands, >= out_offset + nsamp_blk - max_delay]
    (contiguous; allocated [ndm, nbands, nsamp_blk - max_delay] when None).
    One pass over the block for all bands; block, delays, mask, workspace,
    nbits, block_mask and t_origin as for dedisperse_device."""
    return _dedisperse_device(block, delays, max_delay, bands, mask, out, out_offset, workspace, stream, zero_dm, nbits,
                              block_mask, t_origin)


# rt_dedisp_step (include/riptide_amd.h)
DEDISP_STEP_DTYPE = np.dtype([("delays_off", np.uint64), ("out_off", np.uint64), ("out_stride", np.uint64),
                              ("out_offset", np.uint64), ("ndm", np.uint32), ("max_delay", np.uint32),
                              ("downsamp", np.uint32), ("reserved", np.uint32)])
DEDISP_MAX_DOWNSAMP = 256    # RT_DEDISP_MAX_DOWNSAMP


def checked_dedisp_steps(steps):
    """steps as a contiguous one-dimensional DEDISP_STEP_DTYPE array;
    ValueError for anything else."""
    steps = np.asarray(steps)
    if steps.dtype != DEDISP_STEP_DTYPE or steps.ndim != 1:
        raise ValueError("steps must be a one-dimensional array of engine.DEDISP_STEP_DTYPE records")
    return np.ascontiguousarray(steps)


def dedisperse_steps_workspace_bytes(dtype, nsamp_blk, nchans, factors, zero_dm=False, nbits=None):
    """Device workspace bytes of dedisperse_steps_device for a block of this
    shape and steps of these downsampling factors: the rows of
    dedisperse_workspace_bytes, then one float32 area of nchans rows of
    nsamp_blk // f samples for the smallest f > 1, which every decimated step
    reuses."""
    f = np.ascontiguousarray(np.atleast_1d(factors), dtype=np.int64)
    if f.ndim != 1 or (f.size and (f.min() < 1 or f.max() > DEDISP_MAX_DOWNSAMP)):
        raise ValueError(f"every downsamp must be in [1, {DEDISP_MAX_DOWNSAMP}]")
    f = f.astype(np.uint32)
    return _size(_L.rt_dedisperse_steps_workspace_bytes, DEDISP_DTYPES[_dedisp_name(dtype, nbits)], int(nsamp_blk),
                 int(nchans), _lib.ptr(f) if f.size else None, f.size, DEDISP_ZERO_DM if zero_dm else 0)


def dedisperse_steps_check(dtype, nsamp_blk, nchans, steps, delays_len, out_floats, zero_dm=False, nbits=None,
                           t_origin=None):
    """The checks of dedisperse_steps_device on a step table, on the host
    (rt_dedisperse_steps_check; no device): ValueError with the entry point's
    message for what it refuses.  t_origin: the absolute sample of row 0 under
    a block mask that covers the rows (None: no block mask)."""
    steps = checked_dedisp_steps(steps)
    bm = None
    if t_origin is not None:
        cells, fill = np.zeros(1, dtype=np.uint8), np.zeros(8, dtype=np.uint8)
        bm = _lib.BlockMaskStruct(cells.ctypes.data, 1, int(t_origin) + int(nsamp_blk), int(t_origin),
                                  fill.ctypes.data)
    _check(_L.rt_dedisperse_steps_check(DEDISP_DTYPES[_dedisp_name(dtype, nbits)], int(nsamp_blk), int(nchans),
                                        _lib.ptr(steps) if steps.size else None, steps.size, int(delays_len),
                                        int(out_floats), DEDISP_ZERO_DM if zero_dm else 0,
                                        None if bm is None else ctypes.byref(bm)))


def dedisperse_steps_device(block, delays, steps, out, mask=None, workspace=None, stream=None, zero_dm=False,
                            nbits=None, block_mask=None, t_origin=0):
    """Every step of a DM plan from one resident block
    (rt_dedisperse_steps_device): the block goes to channel-major rows once;
    a step of downsamp f > 1 first sums f consecutive samples of every row
    (dedisp_decimate_kernel), then the rows are summed along the step's
    delays, which are in decimated samples (dispersion_delays at tsamp * f):

      z[u, c]   = sum over i < f of block[f * u + i, c]      u < nsamp_blk // f
      out[d, u] = sum over unmasked c of z[u + delay[d, c], c]

    A step of downsamp 1 gives dedisperse_device's bits.  8-bit and 1/2/4-bit
    results without zero_dm are exact integers (vmax * f * nchans must be
    below 2^24); everything else is float32 additions in index order, the
    bits of dedispersion.dedisperse_ds_host.

    delays: one contiguous int32 [rows, nchans] tensor on the block's device
    holding every step's table; steps: DEDISP_STEP_DTYPE records, delays_off
    in int32 elements of `delays`, out_off in floats of `out`, a contiguous
    one-dimensional float32 tensor.  Step k writes out[out_off + d * out_stride
    + out_offset + u] for u < nsamp_blk // downsamp - max_delay; returns the
    list of those [ndm, nout] views of out.  block, mask, nbits, zero_dm,
    block_mask and t_origin (a multiple of every downsamp) as for
    dedisperse_device; the workspace is that of
    dedisperse_steps_workspace_bytes.  Stream-ordered, no host
    synchronisation; ValueError, nothing launched, for what
    rt_dedisperse_steps_check refuses and for a short workspace."""
    import torch
    name, nsamp_blk, nchans = _dedisp_block(block, nbits)
    bm = _block_mask_struct(block_mask, t_origin, block, name, nchans)
    steps = checked_dedisp_steps(steps)
    if (delays.dim() != 2 or delays.dtype != torch.int32 or delays.device != block.device
            or not delays.is_contiguous() or delays.shape[1] != nchans):
        raise ValueError("delays must be a contiguous int32 [ndm, nchans] tensor on the block's device")
    if out.dim() != 1 or out.dtype != torch.float32 or out.device != block.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous one-dimensional float32 tensor on the block's device")
    _check_device_mask(mask, block, nchans)
    flags = DEDISP_ZERO_DM if zero_dm else 0
    with stream_scope(block.device, stream) as (_, handle):
        # the table's own checks, before anything is allocated
        _check(_L.rt_dedisperse_steps_check(DEDISP_DTYPES[name], nsamp_blk, nchans,
                                            _lib.ptr(steps) if steps.size else None, steps.size, delays.numel(),
                                            out.numel(), flags, None if bm is None else ctypes.byref(bm)))
        need = dedisperse_steps_workspace_bytes(name, nsamp_blk, nchans, steps["downsamp"], zero_dm)
        workspace = checked_workspace(workspace, need, block.device, "block", floor=16)
        _check(_L.rt_dedisperse_steps_device(_lib.ptr(block), DEDISP_DTYPES[name], nsamp_blk, nchans,
                                             _lib.ptr(delays), delays.numel(),
                                             None if mask is None else _lib.ptr(mask), _lib.ptr(steps), steps.size,
                                             _lib.ptr(out), out.numel(), _lib.ptr(workspace), workspace.numel(),
                                             handle, flags, None if bm is None else ctypes.byref(bm)))
    return [out.as_strided((int(s["ndm"]), nsamp_blk // int(s["downsamp"]) - int(s["max_delay"])),
                           (int(s["out_stride"]), 1), int(s["out_off"]) + int(s["out_offset"])) for s in steps]


# rt_cutout_spec (include/riptide_amd.h)
CUTOUT_JOB_DTYPE = np.dtype([("start", np.int64), ("out_off", np.uint64), ("factor", np.uint32),
                             ("nbins", np.uint32), ("delay_row", np.uint32), ("band_lo", np.uint32),
                             ("band_hi", np.uint32), ("reserved", np.uint32)])


def checked_cutout_jobs(jobs):
    """jobs as a contiguous one-dimensional CUTOUT_JOB_DTYPE array; ValueError
    for anything else."""
    jobs = np.asarray(jobs)
    if jobs.dtype != CUTOUT_JOB_DTYPE or jobs.ndim != 1:
        raise ValueError("jobs must be a one-dimensional array of engine.CUTOUT_JOB_DTYPE records")
    return np.ascontiguousarray(jobs)


def pulse_cutouts_plan(esize, lo, hi):
    """(tile, ndw, staged) of the cutout kernel (rt_pulse_cutouts_plan; no
    device call): the bins of a tile, and for a channel whose clamped span of
    a tile is the elements [lo, hi) of its row -- esize 1 for 8-bit rows, 4
    for float rows -- the dwords it takes and whether they go through LDS or
    the row is read directly (8-bit rows: staged iff (lo & 3) + hi - lo <=
    4096; float rows: iff hi - lo <= 1024)."""
    tile, ndw, staged = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
    _check(_L.rt_pulse_cutouts_plan(int(esize), int(lo), int(hi), ctypes.byref(tile), ctypes.byref(ndw),
                                    ctypes.byref(staged)))
    return tile.value, ndw.value, bool(staged.value)


def pulse_cutouts_device(block, jobs, delays, max_delay, mask=None, out=None, workspace=None, stream=None,
                         zero_dm=False, nbits=None, block_mask=None, t_origin=0):
    """Dedispersed, time-decimated windows of one resident block, one per job
    (rt_pulse_cutouts_device): jobs is a host array of CUTOUT_JOB_DTYPE, delays
    int32 [R, nchans] on the block's device (entries clamped to [0, max_delay]
    as they are read), and job (start, factor f, nbins T, delay_row, [band_lo,
    band_hi), out_off) writes

      out[out_off + n] = sum over unmasked c in [band_lo, band_hi) and j < f of
                         block[start + n * f + j + delays[delay_row, c], c]

    for n < T; start is relative to the block's row 0 and may be negative, and
    a sample outside the block's rows is skipped.  Returns out, a contiguous
    float32 [>= every out_off + nbins] tensor (allocated to exactly that when
    None).  8-bit sums are exact integers; float sums (float32, 16-bit, and
    everything under zero_dm) are added in channel order, then sample order, and
    equal pulse_candidates.pulse_cutouts_host bit for bit.  block, mask,
    workspace (dedisperse_workspace_bytes), nbits, zero_dm, block_mask and
    t_origin as for dedisperse_device.  Stream-ordered, no host
    synchronisation; no jobs: an empty tensor (or out), nothing launched."""
    import torch
    name, nsamp_blk, nchans = _dedisp_block(block, nbits)
    bm = _block_mask_struct(block_mask, t_origin, block, name, nchans)
    jobs = checked_cutout_jobs(jobs)
    if (delays.dim() != 2 or delays.dtype != torch.int32 or delays.device != block.device
            or not delays.is_contiguous() or delays.shape[1] != nchans):
        raise ValueError("delays must be a contiguous int32 [R, nchans] tensor on the block's device")
    _check_device_mask(mask, block, nchans)
    need_out = int((jobs["out_off"] + jobs["nbins"]).max()) if jobs.size else 0
    with stream_scope(block.device, stream) as (_, handle):
        out = checked_out(out, (need_out,), torch.float32, block.device,
                          f"out must be a contiguous float32 [>= {need_out}] tensor on the block's device",
                          lambda o: (o.dim() != 1 or o.dtype != torch.float32 or o.device != block.device
                                     or not o.is_contiguous() or o.numel() < need_out))
        if not jobs.size:
            return out
        need = dedisperse_workspace_bytes(name, nsamp_blk, nchans, zero_dm)
        workspace = checked_workspace(workspace, need, block.device, "block", floor=16)
        d_jobs = torch.empty(jobs.size * CUTOUT_JOB_DTYPE.itemsize, dtype=torch.uint8, device=block.device)
        _check(_L.rt_pulse_cutouts_device(_lib.ptr(block), DEDISP_DTYPES[name], nsamp_blk, nchans, _lib.ptr(delays),
                                          delays.shape[0], int(max_delay), None if mask is None else _lib.ptr(mask),
                                          _lib.ptr(jobs), jobs.size, _lib.ptr(d_jobs), _lib.ptr(out), out.numel(),
                                          _lib.ptr(workspace), workspace.numel(), handle,
                                          DEDISP_ZERO_DM if zero_dm else 0,
                                          None if bm is None else ctypes.byref(bm)))
    return out


# rt_inject_spec (include/riptide_amd.h)
INJECT_SPEC_DTYPE = np.dtype([("tmpl_off", np.uint64), ("amp_off", np.uint64), ("delay_off", np.uint64),
                              ("step", np.uint64), ("phase0", np.uint64), ("t0", np.int64), ("factor", np.float64),
                              ("span", np.uint64), ("kind", np.uint32), ("log2bins", np.uint32),
                              ("length", np.uint32), ("reserved", np.uint32)])


def inject_device(block, tables, t_origin=0, seed=0, stream=None):
    """Add the signals of an injection.InjectionTables to one resident block,
    in place (rt_inject_device; the specification: injection.inject_host, bit
    for bit): block uint8 / int8 / float32 [nsamp_blk, nchans] (time-major,
    contiguous; a row slice of a larger tensor is fine), whose row 0 is
    absolute sample t_origin of the observation; seed picks the dither of
    8-bit samples.  The tables are uploaded once per InjectionTables and
    device and kept with it.  One launch, stream-ordered, no host
    synchronisation, no workspace.  Packed rows cannot be passed: they are
    uint8 here and would be taken for 8-bit samples (the file-level entry
    points refuse packed files).  ValueError, nothing launched, for a block of
    another channel count than the tables', t_origin + nsamp_blk >= 2^31, and
    a table rt_inject_check refuses.  Returns block."""
    import torch
    name, nsamp_blk, nchans = _dedisp_block(block)
    if nchans != tables.nchans:
        raise ValueError(f"the injection tables have {tables.nchans} channels, the block {nchans}")
    t_origin, seed = int(t_origin), int(seed)
    if t_origin < 0 or not 0 <= seed < 1 << 64:
        raise ValueError("inject: t_origin must not be negative and seed must be in [0, 2^64)")
    # uploaded on the device's current stream, not on `stream`: the tables outlive the call
    d = tables.on_device(block.device)
    with stream_scope(block.device, stream) as (_, handle):
        _check(_L.rt_inject_device(_lib.ptr(block), DEDISP_DTYPES[name], nsamp_blk, nchans, t_origin, seed,
                                   _lib.ptr(tables.specs), tables.specs.size, _lib.ptr(d[0]), _lib.ptr(d[1]),
                                   tables.tmpl.size, _lib.ptr(d[2]), tables.amp.size, _lib.ptr(d[3]),
                                   tables.delay.size, handle))
    return block


def profile_enable(on=True):
    _check(_L.rt_profile_enable(int(bool(on))))


def profile_reset():
    _check(_L.rt_profile_reset())


def profile_read(kind=0):
    """Accumulated (ms, algorithmic bytes, moved bytes, launches) of the cone
    kernel (kind 0) or the downsample ladder (kind 1) since the last reset."""
    ms, alg, mv, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
    _check(_L.rt_profile_read(int(kind), ctypes.byref(ms), ctypes.byref(alg), ctypes.byref(mv), ctypes.byref(n)))
    return {"ms": ms.value, "alg_bytes": alg.value, "moved_bytes": mv.value, "launches": n.value}
