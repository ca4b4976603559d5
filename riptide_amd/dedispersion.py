"""Incoherent dedispersion of channelised data on the GPU: the stage in front
of the periodicity search, so a filterbank file is read once and every DM
trial is produced in device memory (rt_dedisperse_* in include/riptide_amd.h,
kernels in csrc/dedisp_kernels.hip).

  out[d, t] = sum over unmasked channels c of x[t + delay[d, c], c]

with the delay of channel c against the highest frequency of the band

  delay[d, c] = floor(kdm * dm[d] * (f_c ** -2 - f_ref ** -2) / tsamp + 0.5)

8-bit data gives exact integer sums; float32 data is summed in float32.
Packed 1-, 2-, 4- and 16-bit data (nbits=, or a reading.PackedFilterbank; the
format: reading.unpack_samples) stays packed up to the device: 1/2/4-bit data
is unpacked inside the transpose and summed exactly, 16-bit data is converted
exactly and summed in float32 (exact up to 256 channels).

zero_dm=True puts the zero-DM filter (Eatough, Keane & Lyne 2009) in front of
the sum: every time sample first loses its mean over the unmasked channels,

  m[t] = float32(sum over unmasked c of x[t, c] / their number),  y = x - m,

and y is summed in float32 for every sample type (RT_DEDISP_ZERO_DM in
include/riptide_amd.h; rfi.py for the mean series and channel statistics).
"""
import ctypes
import typing

import numpy as np

from . import _lib
from .engine import DEDISP_DTYPES, DEDISP_PACKED_NBITS, DEDISP_ZERO_DM, checked_bands as _checked_bands

_L = _lib.load()
_check = _lib.check

# Dispersion constant in s MHz^2 cm^3 / pc: the rounded value 1 / 2.41e-4 that
# PRESTO, SIGPROC and pulsar timing software share (not the more precise
# 4.148808e3, which would put DMs on a slightly different scale than theirs).
KDM = 1.0 / 2.41e-4

# dedisperse_filterbank refuses a call whose output plus gulp buffers exceeds this
DEFAULT_BUDGET_BYTES = 32 << 30
# default bytes of one gulp of input
DEFAULT_GULP_BYTES = 256 << 20

MAX_CHANS_8BIT = 65793    # RT_DEDISP_MAX_CHANS_8BIT: 255 * nchans < 2^24


def dispersion_delays(freqs, dms, tsamp, kdm=KDM):
    """(delays int64 [ndm, nchans], max_delay) in samples of `tsamp` seconds
    for channel frequencies `freqs` (MHz) and trial DMs `dms` (pc cm^-3),
    against the highest frequency (rt_dedisperse_delays; host only).
    ValueError for an empty input, a frequency that is not positive and finite,
    a DM that is negative or not finite, tsamp <= 0, or a delay of 2^31
    samples or more."""
    freqs = np.ascontiguousarray(np.atleast_1d(freqs), dtype=np.float64)
    dms = np.ascontiguousarray(np.atleast_1d(dms), dtype=np.float64)
    if freqs.ndim != 1 or dms.ndim != 1:
        raise ValueError("freqs and dms must be one-dimensional")
    delays = np.zeros((dms.size, freqs.size), dtype=np.int64)
    md = ctypes.c_int64(0)
    _check(_L.rt_dedisperse_delays(_lib.ptr(freqs), freqs.size, _lib.ptr(dms), dms.size, float(tsamp), float(kdm),
                                   _lib.ptr(delays), ctypes.byref(md)))
    return delays, int(md.value)


def _checked_mask(mask, nchans):
    if mask is None:
        return None
    mask = np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8)
    if mask.shape != (nchans,):
        raise ValueError(f"mask must have one entry per channel ({nchans})")
    return mask


def _checked_packed(data, nbits):
    """(packed rows uint8 [nsamp, row_bytes], type code, nchans) of host data
    given with nbits."""
    nbits = int(nbits)
    data = np.asarray(data)
    if nbits not in DEDISP_PACKED_NBITS:
        raise ValueError("nbits must be 1, 2, 4 or 16")
    if data.ndim != 2 or data.dtype != np.uint8:
        raise ValueError("packed data must be a uint8 array [nsamp, row_bytes]")
    if data.shape[1] * 8 % nbits:
        raise ValueError(f"rows of {data.shape[1]} bytes are not a whole number of {nbits}-bit channels")
    nchans = data.shape[1] * 8 // nbits
    if nbits != 16 and nchans > MAX_CHANS_8BIT:
        raise ValueError(f"{nbits}-bit data with {nchans} channels: sums are exact only up to {MAX_CHANS_8BIT} "
                         "channels (255 * nchans must be below 2^24)")
    return np.ascontiguousarray(data), DEDISP_DTYPES[f"u{nbits}"], nchans


def _host_block(data, nbits):
    """(contiguous array, type code, nsamp, nchans) of a host data argument."""
    if nbits is not None:
        data, code, nchans = _checked_packed(data, nbits)
        return data, code, data.shape[0], nchans
    data = np.ascontiguousarray(_checked_data(data))
    return data, DEDISP_DTYPES[data.dtype.name], data.shape[0], data.shape[1]


def check_max_delay(max_delay, nsamp, what="file"):
    """ValueError unless the `nsamp` samples of the file (or `what`) outlast
    the largest delay of a DM list."""
    if max_delay >= nsamp:
        raise ValueError(f"the largest delay ({max_delay} samples) is not below the {nsamp} samples of the {what}")


def _checked_data(data):
    data = np.asarray(data)
    if data.ndim != 2 or data.dtype.name not in DEDISP_DTYPES:
        raise ValueError("data must be a uint8, int8 or float32 array [nsamp, nchans]")
    if data.dtype != np.float32 and data.shape[1] > MAX_CHANS_8BIT:
        raise ValueError(f"8-bit data with {data.shape[1]} channels: sums are exact only up to {MAX_CHANS_8BIT} "
                         "channels (255 * nchans must be below 2^24)")
    return data


def zero_dm_mean_host(data, mask=None, nbits=None):
    """The zero-DM mean series on the host (rt_zero_dm_mean_host, no device):
    float32 [nsamp], every time sample's mean over the unmasked channels.
    nbits: data is packed rows, as for dedisperse."""
    data, code, nsamp, nchans = _host_block(data, nbits)
    mask = _checked_mask(mask, nchans)
    m = np.zeros(nsamp, dtype=np.float32)
    _check(_L.rt_zero_dm_mean_host(_lib.ptr(data), code, nsamp, nchans,
                                   None if mask is None else _lib.ptr(mask), _lib.ptr(m)))
    return m


def _dedisperse_host(data, delays, max_delay, bands, mask, nout, zero_dm, nbits):
    """dedisperse_host (bands None) and dedisperse_bands_host."""
    data, code, nsamp, nchans = _host_block(data, nbits)
    delays = np.ascontiguousarray(delays, dtype=np.int64)
    if delays.ndim != 2 or delays.shape[1] != nchans:
        raise ValueError("delays must be [ndm, nchans]")
    mask = _checked_mask(mask, nchans)
    if bands is not None:
        bands = np.ascontiguousarray(bands, dtype=np.uint32)
        if bands.ndim != 2 or bands.shape[1] != 2:
            raise ValueError("bands must be [nbands, 2]")
    nout = nsamp - int(max_delay) if nout is None else int(nout)
    if nout < 0:
        raise ValueError(f"max_delay {max_delay} exceeds the {nsamp} samples of the input")
    ndm = delays.shape[0]
    out = np.zeros((ndm, nout) if bands is None else (ndm, bands.shape[0], nout), dtype=np.float32)
    head = (_lib.ptr(data), code, nsamp, nchans, _lib.ptr(delays), None if mask is None else _lib.ptr(mask), ndm)
    tail = (int(max_delay), nout, _lib.ptr(out), DEDISP_ZERO_DM if zero_dm else 0)
    if bands is None:
        _check(_L.rt_dedisperse_host_opt(*head, *tail))
    else:
        _check(_L.rt_dedisperse_bands_host(*head, _lib.ptr(bands), bands.shape[0], *tail))
    return out


def dedisperse_host(data, delays, max_delay, mask=None, nout=None, zero_dm=False, nbits=None):
    """The specification on the host (rt_dedisperse_host_opt, no device):
    float32 [ndm, nout] from data [nsamp, nchans] and a delay table; nout
    defaults to nsamp - max_delay.  nbits: data is packed rows, as for
    dedisperse."""
    return _dedisperse_host(data, delays, max_delay, None, mask, nout, zero_dm, nbits)


def _dedisperse(data, freqs, tsamp, dms, bands, mask, kdm, zero_dm, nbits):
    """dedisperse (bands None) and dedisperse_bands."""
    data, code, nsamp, nchans = _host_block(data, nbits)
    delays, max_delay = dispersion_delays(freqs, dms, tsamp, kdm)
    if delays.shape[1] != nchans:
        raise ValueError("freqs must have one entry per channel of data")
    mask = _checked_mask(mask, nchans)
    if bands is not None:
        bands = _checked_bands(bands, nchans)
    check_max_delay(max_delay, nsamp, "data")
    ndm, nout = delays.shape[0], nsamp - max_delay
    out = np.empty((ndm, nout) if bands is None else (ndm, bands.shape[0], nout), dtype=np.float32)
    head = (_lib.ptr(data), code, nsamp, nchans, _lib.ptr(delays), None if mask is None else _lib.ptr(mask), ndm)
    tail = (max_delay, _lib.ptr(out), DEDISP_ZERO_DM if zero_dm else 0)
    if bands is None:
        _check(_L.rt_dedisperse_opt(*head, *tail))
    else:
        _check(_L.rt_dedisperse_bands(*head, _lib.ptr(bands), bands.shape[0], *tail))
    return out


def dedisperse(data, freqs, tsamp, dms, mask=None, kdm=KDM, zero_dm=False, nbits=None):
    """Dedisperse host data [nsamp, nchans] (uint8, int8 or float32) at the
    trial DMs on the GPU: float32 [ndm, nsamp - max_delay] (rt_dedisperse:
    upload, kernels, download).  mask: per channel, True = skipped; a masked
    channel still counts towards the reference frequency and max_delay.
    nbits (1, 2, 4 or 16): data is packed rows instead, uint8 [nsamp,
    nchans * nbits / 8] (reading.pack_samples / unpack_samples)."""
    return _dedisperse(data, freqs, tsamp, dms, None, mask, kdm, zero_dm, nbits)


def band_edges(nchans, nsub):
    """uint32 [nsub, 2]: the channel ranges [lo, hi) of nsub contiguous
    sub-bands of nchans channels, lo_s = s * nchans // nsub and hi_s =
    (s + 1) * nchans // nsub (no band empty, widths differing by at most one
    channel).  ValueError unless 1 <= nsub <= nchans."""
    nchans, nsub = int(nchans), int(nsub)
    if not 1 <= nsub <= nchans:
        raise ValueError(f"nsub must be in [1, {nchans}], the number of channels")
    edges = np.arange(nsub + 1, dtype=np.int64) * nchans // nsub
    return np.stack([edges[:-1], edges[1:]], axis=1).astype(np.uint32)


def dedisperse_bands_host(data, delays, max_delay, bands, mask=None, nout=None, zero_dm=False, nbits=None):
    """The specification of the band sums on the host (rt_dedisperse_bands_host,
    no device): float32 [ndm, nbands, nout],

      out[d, b, t] = sum over unmasked c in [lo_b, hi_b) of x[t + delay[d, c], c]

    for bands uint32 [nbands, 2] of channel ranges [lo, hi), which may overlap,
    be empty or cover the whole file.  Everything else as dedisperse_host; with
    zero_dm the mean is over the unmasked channels of the whole file."""
    return _dedisperse_host(data, delays, max_delay, bands, mask, nout, zero_dm, nbits)


def dedisperse_bands(data, freqs, tsamp, dms, bands, mask=None, kdm=KDM, zero_dm=False, nbits=None):
    """dedisperse() for every band of a table on the GPU: float32
    [ndm, nbands, nsamp - max_delay] (rt_dedisperse_bands: upload, kernels,
    download).  The delays are against the highest frequency of all of
    `freqs`, whatever the bands."""
    return _dedisperse(data, freqs, tsamp, dms, bands, mask, kdm, zero_dm, nbits)


def _checked_sample_type(fb):
    """nbits of a reading.PackedFilterbank, None for a Filterbank; ValueError
    for samples no entry point takes."""
    nbits = getattr(fb, "nbits", None)
    if nbits is None and np.dtype(fb.dtype).name not in DEDISP_DTYPES:
        raise ValueError("the filterbank's samples must be uint8, int8 or float32")
    if nbits is not None and nbits not in DEDISP_PACKED_NBITS:
        raise ValueError("a packed filterbank must hold 1-, 2-, 4- or 16-bit samples")
    return nbits


def _gulp_layout(fb):
    """(elements of a row of fb.data, their numpy dtype): the raw bytes of a
    PackedFilterbank, the samples of a Filterbank."""
    nbits = getattr(fb, "nbits", None)
    if nbits is not None:
        return fb.row_bytes, np.dtype(np.uint8)
    return fb.nchans, np.dtype(fb.dtype)


def _block_mask_bytes(fb, block_mask):
    """Device bytes of a block mask's cells and fill for this file (0 for None)."""
    if block_mask is None:
        return 0
    nbits = getattr(fb, "nbits", None)
    esize = 2 if nbits == 16 else 1 if nbits is not None else np.dtype(fb.dtype).itemsize
    return int(block_mask.cells.size) + int(block_mask.cells.shape[1]) * esize


def _upload_block_mask(fb, block_mask, dev, nrows):
    """A rfi.BlockMask as the engine.DeviceBlockMask of file `fb` on `dev`:
    the cells as uint8 and the fill in the file's sample type, uploaded once
    for every gulp of a call that reads rows [0, nrows).  None for None.
    ValueError when the mask's channel count is not the file's, or its blocks
    do not cover the rows read."""
    if block_mask is None:
        return None
    import torch
    from . import engine
    cells = np.asarray(block_mask.cells)
    if cells.ndim != 2 or cells.shape[1] != fb.nchans:
        raise ValueError(f"the block mask has {cells.shape[1] if cells.ndim == 2 else '?'} channels, the file "
                         f"{fb.nchans}")
    block_len = int(block_mask.block_len)
    if block_len < 1:
        raise ValueError("block_mask: block_len must be at least 1")
    if cells.shape[0] * block_len < nrows:
        raise ValueError(f"the block mask covers {cells.shape[0]} blocks of {block_len} samples, fewer than the "
                         f"{nrows} samples read")
    fill = np.ascontiguousarray(block_mask.typed_fill(fb))
    d_cells = torch.from_numpy(np.ascontiguousarray(cells.astype(bool), dtype=np.uint8)).to(dev)
    return engine.DeviceBlockMask(d_cells, torch.from_numpy(fill).to(dev), block_len)


def _resolve_inject(inject, fb):
    """(tables, seed) of an inject= argument checked against `fb`, None for
    None (injection.resolve_inject, imported on first use: that module imports
    this one)."""
    if inject is None:
        return None
    from .injection import resolve_inject
    return resolve_inject(inject, fb)


def stream_gulps(fb, dev, gulp, nrows, overlap, process):
    """Stream rows [0, nrows) of a reading.Filterbank's memory map to `dev` in
    gulps of `gulp` time samples that overlap by `overlap`, through two
    page-locked staging buffers and two device blocks: the upload of gulp
    k + 1 runs on a copy stream behind the kernels of gulp k.  For every gulp
    process(block, start) queues its kernels on the current stream; block is
    the device tensor [g, nchans] of rows [start, start + g) -- for a
    reading.PackedFilterbank the packed rows, uint8 [g, row_bytes]; the gulp is
    counted in time samples either way.  Called inside
    torch.cuda.device(dev); returns once the last gulp is queued and every
    upload is done.  (dedisperse_filterbank, rfi.channel_stats and
    rfi.zero_dm_series share it.)"""
    import torch
    nchans, tdtype = _gulp_layout(fb)
    tdtype = {"uint8": torch.uint8, "int8": torch.int8, "float32": torch.float32}[tdtype.name]
    main = torch.cuda.current_stream(dev)
    copy = torch.cuda.Stream(device=dev)
    pinned = [torch.empty((gulp, nchans), dtype=tdtype).pin_memory() for _ in range(2)]
    blocks = [torch.empty((gulp, nchans), dtype=tdtype, device=dev) for _ in range(2)]
    uploaded = [torch.cuda.Event() for _ in range(2)]   # slot's upload is done: its staging buffer is free
    consumed = [torch.cuda.Event() for _ in range(2)]   # slot's kernels are done: its device block is free
    # The device blocks come from the main stream's pool: the allocator may
    # hand out memory that work already queued on main (an earlier call's
    # last kernels, say) still reads.  The copy stream starts behind it.
    copy.wait_stream(main)
    start, k = 0, 0
    while start < nrows - overlap:
        g = min(gulp, nrows - start)
        slot = k & 1
        if k >= 2:
            uploaded[slot].synchronize()
        np.copyto(pinned[slot][:g].numpy(), fb.data[start:start + g])
        with torch.cuda.stream(copy):
            if k >= 2:
                copy.wait_event(consumed[slot])
            blocks[slot][:g].copy_(pinned[slot][:g], non_blocking=True)
            uploaded[slot].record(copy)
        main.wait_event(uploaded[slot])
        process(blocks[slot][:g], start)
        consumed[slot].record(main)
        start += g - overlap
        k += 1
    # Every upload is done before the staging buffers and the device blocks
    # are released with this frame, so the copy stream no longer uses
    # them; the kernels still queued read the blocks on main, the stream
    # the blocks were allocated on, whose pool reuses them in stream order.
    uploaded[(k - 1) & 1].synchronize()
    if k > 1:
        uploaded[k & 1].synchronize()


def dedisperse_filterbank(fb, dms, mask=None, gulp=None, device=None, kdm=KDM, nout=None,
                          budget_bytes=DEFAULT_BUDGET_BYTES, zero_dm=False, bands=None, block_mask=None, inject=None):
    """Dedisperse a reading.Filterbank (or PackedFilterbank: the rows are
    uploaded packed) at the trial DMs into one device tensor
    float32 [ndm, nout], nout = nsamp - max_delay (or a smaller `nout`: the
    first nout samples, e.g. the length a larger DM list would leave).

    The memory map is streamed in gulps of `gulp` time samples (default: about
    256 MiB of input, at least 2 * max_delay + 1) that overlap by max_delay,
    through two page-locked staging buffers: the upload of gulp k + 1 runs on a
    copy stream behind the kernels of gulp k.  The result does not depend on
    gulp.  Queued on the current stream of `device`; the call returns once the
    last gulp is queued.

    zero_dm: the zero-DM filter in front of the sum (module docstring).  The
    mean of a time sample needs that sample's row alone, so the result still
    does not depend on gulp; the workspace of a gulp is the larger float32 one.

    bands (uint32 [nbands, 2] of channel ranges [lo, hi): band_edges): the
    result is float32 [ndm, nbands, nout] instead, every band's sum of every DM
    from the same single pass over the file (engine.dedisperse_bands_device),
    and the output counted against the budget is ndm * nbands * nout * 4 bytes.

    block_mask (a rfi.BlockMask, from rfi.block_mask(rfi.block_stats(fb))): a
    mask in time and frequency.  Every sample of a flagged cell is replaced by
    its channel's fill in the file's sample type as the block is read on the
    device, in front of everything above (the channel mask, the zero-DM mean,
    the sums): the result is that of the same call on a file holding the
    replaced samples (rfi.apply_block_mask_host), bit for bit, and does not
    depend on gulp.  The cells and the fill are uploaded once and count
    against the budget.

    inject (an injection.InjectionTables, or (tables, seed)): synthetic
    signals are added to every gulp's block in place as it arrives on the
    device (engine.inject_device), in front of the block mask and everything
    behind it: the result is that of the same call on a file holding
    injection.inject_host's samples, bit for bit, and does not depend on gulp
    (overlap rows are uploaded afresh with every gulp and the injected value
    depends on the absolute sample alone).  Packed files are refused.  The
    tables (a few KiB per signal, uploaded once and kept with the
    InjectionTables) are not counted against the budget, so a call fits it
    with inject= exactly when it fits without.

    ValueError -- nothing is launched -- when max_delay >= nsamp, for 8-bit
    data of more than 65793 channels, for a block mask of another channel
    count or one that does not cover the rows read, and when the output (ndm *
    nout * 4 bytes) plus the gulp buffers exceed budget_bytes: pass fewer DMs
    per call."""
    import torch
    from . import engine
    from ._args import resolve_device
    inject = _resolve_inject(inject, fb)
    dev = resolve_device(device)
    nsamp, nchans = fb.nsamp, fb.nchans
    nbits = _checked_sample_type(fb)
    row_elems, dtype = _gulp_layout(fb)
    if (dtype != np.float32 and nbits != 16) and nchans > MAX_CHANS_8BIT:
        raise ValueError(f"8-bit data with {nchans} channels: sums are exact only up to {MAX_CHANS_8BIT} channels "
                         "(255 * nchans must be below 2^24)")
    delays, max_delay = dispersion_delays(fb.freqs, dms, fb.tsamp, kdm)
    mask = _checked_mask(mask, nchans)
    check_max_delay(max_delay, nsamp)
    full = nsamp - max_delay
    nout = full if nout is None else int(nout)
    if not 0 < nout <= full:
        raise ValueError(f"nout must be in [1, {full}]")
    ndm = delays.shape[0]
    row_bytes = row_elems * dtype.itemsize
    if gulp is None:
        gulp = max(DEFAULT_GULP_BYTES // row_bytes, 2 * max_delay + 1)
    gulp = int(gulp)
    if gulp <= max_delay:
        raise ValueError(f"gulp must exceed the largest delay ({max_delay} samples)")
    need_in = nout + max_delay          # input rows the outputs read
    gulp = min(gulp, need_in)
    ws_bytes = engine.dedisperse_workspace_bytes(dtype.name, gulp, nchans, zero_dm, nbits=nbits)
    if bands is not None:
        bands = _checked_bands(bands, nchans)
    out_bytes = ndm * (1 if bands is None else bands.shape[0]) * nout * 4
    total = out_bytes + 2 * gulp * row_bytes + ws_bytes + _block_mask_bytes(fb, block_mask)
    if total > int(budget_bytes):
        raise ValueError(f"dedispersing {ndm} DMs needs {total} bytes of device memory ({out_bytes} of output "
                         f"plus the gulp buffers), over the budget of {int(budget_bytes)}: pass fewer DMs per call")
    with torch.cuda.device(dev):
        d_delays = torch.from_numpy(delays.astype(np.int32)).to(dev)
        d_mask = None if mask is None else torch.from_numpy(mask).to(dev)
        workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        out = torch.empty((ndm, nout) if bands is None else (ndm, bands.shape[0], nout), dtype=torch.float32,
                          device=dev)
        d_bands = None if bands is None else torch.from_numpy(bands.view(np.int32)).to(dev)
        d_bm = _upload_block_mask(fb, block_mask, dev, need_in)

        def process(block, start):
            if inject is not None:
                engine.inject_device(block, inject[0], start, inject[1])
            # dedisperse_device, or with a table dedisperse_bands_device
            engine._dedisperse_device(block, d_delays, max_delay, d_bands, d_mask, out, start, workspace, None,
                                      zero_dm, nbits, d_bm, start)

        stream_gulps(fb, dev, gulp, need_in, max_delay, process)
    return out


def band_series(fb, dms, bands, deredden_params, nout, mask=None, zero_dm=False, kdm=KDM, device=None,
                budget_bytes=DEFAULT_BUDGET_BYTES, block_mask=None):
    """The series a candidate's frequency-phase diagnostic is folded from:
    (device tensor float32 [ndm, nbands, nout], bool [nbands]).  The file is
    dedispersed into every band at every DM by one pass
    (dedisperse_filterbank(..., bands=bands, nout=nout)), then every row is
    dereddened (deredden_params: rmed_width in seconds, rmed_minpts) and
    normalised by one batched engine.deredden_normalise call, as the search
    does with a DM trial.  The second result marks the bands with no unmasked
    channel: their rows are left zero and are not normalised (the variance of
    a constant row is zero).  block_mask as for dedisperse_filterbank."""
    import torch
    from . import engine
    bands = _checked_bands(bands, fb.nchans)
    mask = _checked_mask(mask, fb.nchans)
    live = np.ones(fb.nchans, dtype=bool) if mask is None else mask == 0
    empty = np.array([not live[lo:hi].any() for lo, hi in bands], dtype=bool)
    raw = dedisperse_filterbank(fb, dms, mask=mask, device=device, kdm=kdm, nout=nout, budget_bytes=budget_bytes,
                                zero_dm=zero_dm, bands=bands, block_mask=block_mask)
    ndm, nbands, nout = raw.shape
    width = int(round(deredden_params["rmed_width"] / fb.tsamp))
    minpts = int(deredden_params["rmed_minpts"])
    rows = raw.view(ndm * nbands, nout)
    with torch.cuda.device(raw.device):
        if not empty.any():
            return engine.deredden_normalise(rows, width, minpts).view(ndm, nbands, nout), empty
        out = torch.zeros_like(rows)
        if not empty.all():
            keep = np.flatnonzero(np.tile(~empty, ndm))
            idx = torch.from_numpy(keep).to(raw.device)
            out[idx] = engine.deredden_normalise(rows[idx], width, minpts)
    return out.view(ndm, nbands, nout), empty


# ---------------------------------------------------------------- the DM plan
MAX_DOWNSAMP = 256    # RT_DEDISP_MAX_DOWNSAMP: the largest factor of a step


class DMStep(typing.NamedTuple):
    """Consecutive trials of a plan that share one decimation factor."""
    dms: np.ndarray       # float64, ascending as planned
    downsamp: int         # f: samples summed per output sample
    tsamp: float          # f * the file's sampling time, seconds (None when built by hand without one)


class DMPlan:
    """Which DMs to search and at what time resolution: `steps` (DMStep), the
    flat `dms` in plan order, the per-trial `downsamp` array, len() = the
    number of trials.  `dm_cover`, the largest DM of the plan this one was cut
    from (shard keeps it), fixes the stretch of the observation every step
    covers, so a sharded plan gives the series of the whole plan.

    dm_plan makes one from a band; DMPlan.from_steps([(dms, downsamp), ...])
    builds one by hand, with any integer downsamp in [1, 256] (dm_plan itself
    only gives powers of two)."""

    def __init__(self, steps, tsamp=None, dm_cover=None):
        self.tsamp = None if tsamp is None else float(tsamp)
        self.steps = []
        for dms, f in steps:
            dms = np.ascontiguousarray(np.atleast_1d(dms), dtype=np.float64)
            if int(f) != f or not 1 <= int(f) <= MAX_DOWNSAMP:
                raise ValueError(f"downsamp {f} must be an integer in [1, {MAX_DOWNSAMP}]")
            if dms.ndim != 1 or not np.all(np.isfinite(dms)) or np.any(dms < 0):
                raise ValueError("the DMs of a step must be a one-dimensional list of non-negative finite numbers")
            if dms.size:
                self.steps.append(DMStep(dms, int(f), None if tsamp is None else int(f) * self.tsamp))
        largest = max((float(s.dms.max()) for s in self.steps), default=0.0)
        self.dm_cover = largest if dm_cover is None else float(dm_cover)
        if self.dm_cover < largest:
            raise ValueError("dm_cover is below the plan's largest DM")

    @classmethod
    def from_steps(cls, steps, tsamp=None):
        return cls(steps, tsamp)

    @property
    def dms(self):
        return np.concatenate([s.dms for s in self.steps]) if self.steps else np.empty(0, dtype=np.float64)

    @property
    def downsamp(self):
        return (np.concatenate([np.full(s.dms.size, s.downsamp, dtype=np.int64) for s in self.steps])
                if self.steps else np.empty(0, dtype=np.int64))

    def __len__(self):
        return sum(s.dms.size for s in self.steps)

    def shard(self, rank, size):
        """The round-robin share of every step (trials rank, rank + size, ...
        of each), empty steps dropped; dm_cover is kept."""
        rank, size = int(rank), int(size)
        if not 0 <= rank < size:
            raise ValueError("rank must be in [0, size)")
        return DMPlan([(s.dms[rank::size], s.downsamp) for s in self.steps], self.tsamp, self.dm_cover)

    def shard_indices(self, rank, size):
        """Indices into the flat `dms` of the trials shard(rank, size) keeps, in its order."""
        idx, first = [], 0
        for s in self.steps:
            idx.extend(range(first + int(rank), first + s.dms.size, int(size)))
            first += s.dms.size
        return idx

    def __repr__(self):
        return "DMPlan(" + ", ".join(f"{s.dms.size} x f={s.downsamp}" for s in self.steps) + ")"


def dm_plan(freqs, tsamp, dm_max, dm_min=0.0, wmin=1.0e-3, oversample=2.0, max_downsamp=64, kdm=KDM):
    """The DM trials of a band and each one's time decimation (rt_dm_plan; host
    only, float64): a DMPlan.

    freqs are the channel centre frequencies in MHz (ascending or descending,
    at least 2).  With cw the channel width, flo / fhi the band edges and fmid
    the band centre, kdisp = kdm (flo^-2 - fhi^-2), ksmear = kdm ((fmid -
    cw/2)^-2 - (fmid + cw/2)^-2), the smearing of a trial is s(DM) = max(wmin,
    ksmear DM) and its coverage radius r(DM) = s(DM) / kdisp -- the quantities
    of the reference's dmiter.select_dms, which thins an existing set of
    trials by the same rule.  The first trial is dm_min; each next trial is
    the DM whose radius touches the previous one's; the last is the first
    whose radius reaches dm_max.  A trial's decimation f is the largest power
    of two <= max_downsamp with f * tsamp * oversample <= s(DM), at least 1;
    consecutive trials of equal f form a DMStep.

    wmin (seconds) is the narrowest pulse searched for.  oversample = 2.0
    (decimated samples across the smearing time) and max_downsamp = 64 are
    interface defaults, not tuned values: nothing was measured to choose them.

    Out of scope: factors that are not powers of two (DMPlan.from_steps and
    the kernels take them).  ValueError for fewer than 2 channels, inputs that
    are not positive and finite (dm_min may be 0), dm_max < dm_min, and more
    than 2^20 trials."""
    freqs = np.ascontiguousarray(np.atleast_1d(freqs), dtype=np.float64)
    if freqs.ndim != 1:
        raise ValueError("freqs must be one-dimensional")
    if int(max_downsamp) != max_downsamp or not 1 <= int(max_downsamp) <= MAX_DOWNSAMP:
        raise ValueError(f"max_downsamp must be an integer in [1, {MAX_DOWNSAMP}]")
    args = (_lib.ptr(freqs), freqs.size, float(tsamp), float(dm_min), float(dm_max), float(wmin), float(oversample),
            int(max_downsamp), float(kdm))
    n = ctypes.c_size_t(0)
    _check(_L.rt_dm_plan(*args, None, None, 0, ctypes.byref(n)))
    dms = np.zeros(n.value, dtype=np.float64)
    f = np.zeros(n.value, dtype=np.uint32)
    _check(_L.rt_dm_plan(*args, _lib.ptr(dms), _lib.ptr(f), n.value, ctypes.byref(n)))
    cuts = np.flatnonzero(np.diff(f.astype(np.int64))) + 1
    return DMPlan([(part, int(ff[0])) for part, ff in zip(np.split(dms, cuts), np.split(f, cuts))], tsamp)


def dedisperse_ds_host(data, delays, max_delay, downsamp, mask=None, nout=None, zero_dm=False, nbits=None,
                       block_mask=None, t_origin=0):
    """The specification of a decimated step on the host
    (rt_dedisperse_ds_host, no device): float32 [ndm, nout],

      z[u, c]   = sum over i < f of x'[f * u + i, c]            u < nsamp // f
      out[d, u] = sum over unmasked c of z[u + delays[d, c], c]

    both sums float32 additions from 0.0f in index order (8-bit and 1/2/4-bit
    data without zero_dm: exact integers; refused when vmax * f * nchans >=
    2^24).  delays are in decimated samples (dispersion_delays at tsamp * f);
    nout defaults to nsamp // f - max_delay.  block_mask: a (cells uint8
    [nblocks, nchans], fill, block_len) triple in host memory, with t_origin a
    multiple of f.  downsamp = 1 is dedisperse_host."""
    data, code, nsamp, nchans = _host_block(data, nbits)
    delays = np.ascontiguousarray(delays, dtype=np.int64)
    if delays.ndim != 2 or delays.shape[1] != nchans:
        raise ValueError("delays must be [ndm, nchans]")
    mask = _checked_mask(mask, nchans)
    f = int(downsamp)
    if not 1 <= f <= MAX_DOWNSAMP:
        raise ValueError(f"dedisperse: downsamp {f} is outside [1, {MAX_DOWNSAMP}]")
    nout = nsamp // f - int(max_delay) if nout is None else int(nout)
    if nout < 0:
        raise ValueError(f"max_delay {max_delay} exceeds the {nsamp // f} decimated samples of the input")
    bm = None
    if block_mask is not None:
        cells, fill, block_len = block_mask
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        fill = np.ascontiguousarray(fill)
        bm = _lib.BlockMaskStruct(cells.ctypes.data, cells.shape[0], int(block_len), int(t_origin), fill.ctypes.data)
    out = np.zeros((delays.shape[0], nout), dtype=np.float32)
    _check(_L.rt_dedisperse_ds_host(_lib.ptr(data), code, nsamp, nchans, _lib.ptr(delays),
                                    None if mask is None else _lib.ptr(mask), delays.shape[0], int(max_delay), f, nout,
                                    _lib.ptr(out), DEDISP_ZERO_DM if zero_dm else 0,
                                    None if bm is None else ctypes.byref(bm)))
    return out


def dedisperse_steps(data, delays, steps, out, mask=None, zero_dm=False, nbits=None):
    """The steps of a step table from host data on the GPU (rt_dedisperse_steps:
    upload, the kernels of engine.dedisperse_steps_device, download;
    synchronous), as dedisperse is for one delay table.  data as for
    dedisperse; delays int64 [rows, nchans] holding every step's table, each
    entry in [0, its step's max_delay]; steps engine.DEDISP_STEP_DTYPE records
    (delays_off in elements of delays, out_off in floats of out); out a
    contiguous one-dimensional float32 array, which is uploaded first, so a
    float no step writes comes back as it was.  Returns the [ndm, nout] views
    of out, one per step.  No block mask."""
    from . import engine
    data, code, nsamp, nchans = _host_block(data, nbits)
    delays = np.ascontiguousarray(delays, dtype=np.int64)
    if delays.ndim != 2 or delays.shape[1] != nchans:
        raise ValueError("delays must be [rows, nchans]")
    steps = engine.checked_dedisp_steps(steps)
    if not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.ndim != 1 or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous one-dimensional float32 array")
    mask = _checked_mask(mask, nchans)
    _check(_L.rt_dedisperse_steps(_lib.ptr(data), code, nsamp, nchans, _lib.ptr(delays), delays.size,
                                  None if mask is None else _lib.ptr(mask), _lib.ptr(steps) if steps.size else None,
                                  steps.size, _lib.ptr(out), out.size, DEDISP_ZERO_DM if zero_dm else 0))
    return [np.lib.stride_tricks.as_strided(
        out[int(s["out_off"]) + int(s["out_offset"]):],
        (int(s["ndm"]), nsamp // int(s["downsamp"]) - int(s["max_delay"])), (int(s["out_stride"]) * 4, 4))
        for s in steps]


def plan_layout(fb, plan, kdm=KDM):
    """Where dedisperse_filterbank_plan puts the steps of `plan` for file `fb`
    (host only): a list, one entry per step, of (delays int64 [ndm, nchans] in
    decimated samples, max_delay, nout).  With D the largest delay at the
    file's own sampling time of plan.dm_cover and L = nsamp - D, nout = min(L
    // f, nsamp // f - max_delay): every step covers the same stretch of the
    observation, whatever share of the plan it is.  ValueError when a step
    leaves no output, and when the plan was made for another sampling time
    than the file's (plan.tsamp, where it is set): its factors were chosen
    against that one."""
    if plan.tsamp is not None and abs(plan.tsamp - fb.tsamp) > 1e-9 * fb.tsamp:
        raise ValueError(f"the plan was made for a sampling time of {plan.tsamp} s, the file has {fb.tsamp} s")
    _, D = dispersion_delays(fb.freqs, [plan.dm_cover], fb.tsamp, kdm)
    check_max_delay(D, fb.nsamp)
    L = fb.nsamp - D
    layout = []
    for s in plan.steps:
        delays, md = dispersion_delays(fb.freqs, s.dms, fb.tsamp * s.downsamp, kdm)
        nout = min(L // s.downsamp, fb.nsamp // s.downsamp - md)
        if nout < 1:
            raise ValueError(f"the step at downsamp {s.downsamp} leaves no output: the largest delay ({md} decimated "
                             f"samples) is not below the {fb.nsamp // s.downsamp} decimated samples of the file")
        layout.append((delays, md, nout))
    return layout


def _plan_setup(fb, plan, gulp, kdm, zero_dm, block_mask):
    """What dedisperse_filterbank_plan works out on the host before anything is
    allocated, as a dict: the layout, the gulp and its overlap, the step table
    of the first gulp (checked), and the device bytes of the call."""
    import math
    from . import engine
    nchans = fb.nchans
    nbits = _checked_sample_type(fb)
    row_elems, dtype = _gulp_layout(fb)
    layout = plan_layout(fb, plan, kdm)
    factors = [s.downsamp for s in plan.steps]
    lcm = 1
    for f in factors:
        lcm = lcm * f // math.gcd(lcm, f)
    # rows the outputs read, a whole number of every step's decimated samples
    need_in = max((nout + md) * f for (_, md, nout), f in zip(layout, factors))
    overlap = -(-max(md * f for (_, md, _), f in zip(layout, factors)) // lcm) * lcm
    row_bytes = row_elems * dtype.itemsize
    if gulp is None:
        gulp = max(DEFAULT_GULP_BYTES // row_bytes, 2 * overlap + lcm)
    gulp = int(gulp) // lcm * lcm
    if gulp <= overlap:
        raise ValueError(f"gulp must be a multiple of {lcm} above the overlap of {overlap} samples")
    if gulp >= need_in:
        gulp = need_in          # one gulp: it may end inside a decimated sample, whose tail is dropped
    name = engine._dedisp_name(dtype.name, nbits)
    # Every gulp writes all the outputs its rows allow, and the rows read end at need_in for every step: a
    # step's rows are allocated cap = need_in // f - max_delay long, the outputs the last gulp reaches, and
    # the result is their first nout columns
    table = np.zeros(len(factors), dtype=engine.DEDISP_STEP_DTYPE)
    row0 = off = 0
    for k, ((delays, md, nout), f) in enumerate(zip(layout, factors)):
        cap = need_in // f - md
        table[k] = (row0 * nchans, off, cap, 0, delays.shape[0], md, f, 0)
        row0 += delays.shape[0]
        off += delays.shape[0] * cap
    # the table of the first gulp, checked before anything is allocated (the exactness cap among the checks)
    engine.dedisperse_steps_check(name, gulp, nchans, table, row0 * nchans, off, zero_dm)
    ws_bytes = engine.dedisperse_steps_workspace_bytes(name, gulp, nchans, factors, zero_dm)
    total = off * 4 + 2 * gulp * row_bytes + ws_bytes + _block_mask_bytes(fb, block_mask)
    return dict(layout=layout, factors=factors, need_in=need_in, overlap=overlap, gulp=gulp, nbits=nbits,
                table=table, out_floats=off, ws_bytes=ws_bytes, total=total)


def plan_device_bytes(fb, plan, gulp=None, kdm=KDM, zero_dm=False, block_mask=None):
    """The device bytes dedisperse_filterbank_plan needs for this plan, what
    it sets against budget_bytes: every step's rows, the two gulp buffers, the
    workspace and the block mask (host only; 0 for an empty plan)."""
    return _plan_setup(fb, plan, gulp, kdm, zero_dm, block_mask)["total"] if plan.steps else 0


def plan_slices(fb, plan, budget_bytes=DEFAULT_BUDGET_BYTES, chunk=8, **kwargs):
    """`plan` cut, in plan order, into the fewest consecutive plans whose
    dedisperse_filterbank_plan fits budget_bytes each (plan_device_bytes,
    which takes kwargs), grown `chunk` trials at a time.  Every slice keeps
    the plan's dm_cover, so its series are the whole plan's.  ValueError when
    `chunk` trials alone do not fit."""
    trials = list(zip(plan.dms, plan.downsamp))
    chunk = max(1, int(chunk))

    def cut(i0, i1):
        steps = []
        for dm, f in trials[i0:i1]:
            if steps and steps[-1][1] == f:
                steps[-1][0].append(dm)
            else:
                steps.append(([dm], int(f)))
        return DMPlan(steps, plan.tsamp, plan.dm_cover)

    slices, i0 = [], 0
    while i0 < len(trials):
        i1 = min(i0 + chunk, len(trials))
        best = cut(i0, i1)
        need = plan_device_bytes(fb, best, **kwargs)
        if need > int(budget_bytes):
            raise ValueError(f"dedispersing {i1 - i0} DMs of the plan needs {need} bytes of device memory, over the "
                             f"budget of {int(budget_bytes)}")
        while i1 < len(trials):
            nxt = cut(i0, min(i1 + chunk, len(trials)))
            if plan_device_bytes(fb, nxt, **kwargs) > int(budget_bytes):
                break
            best, i1 = nxt, min(i1 + chunk, len(trials))
        slices.append(best)
        i0 = i1
    return slices


def dedisperse_filterbank_plan(fb, plan, mask=None, gulp=None, device=None, kdm=KDM,
                               budget_bytes=DEFAULT_BUDGET_BYTES, zero_dm=False, block_mask=None, inject=None):
    """Dedisperse a reading.Filterbank or PackedFilterbank at every trial of a
    DMPlan, each step decimated in time by its factor f: a list of device
    tensors, one float32 [ndm_step, nout_step] per step, at the sampling time
    f * fb.tsamp.  Decimation comes first and the sum second (the
    specification: dedisperse_ds_host); a step of f = 1 gives
    dedisperse_filterbank's bits.  nout_step is plan_layout's: every step
    covers the same stretch of the observation, so the result does not depend
    on how a plan was sharded.

    The file is streamed once (stream_gulps) for all steps: every gulp goes to
    channel-major rows once and every step is decimated and summed from those
    (engine.dedisperse_steps_device).  The gulp is rounded down to a multiple
    of the least common multiple of the factors and gulps overlap by the
    largest max_delay * f rounded up to that multiple, so every gulp starts on
    a decimated sample of every step and the result does not depend on gulp.
    The step tensors are views of one allocation, rows with unit sample
    stride and a row stride of at least nout_step.

    mask, zero_dm, block_mask and inject as for dedisperse_filterbank (the
    injection comes first, at the file's resolution).  Out of scope:
    bands= (sub-band sums stay at the file's resolution) and pulses.
    ValueError -- nothing is launched -- for what dedisperse_filterbank
    refuses, for vmax * f * nchans >= 2^24 of integer data, for a gulp not
    above the overlap, and when all step outputs plus the gulp buffers and the
    workspace exceed budget_bytes."""
    import torch
    from . import engine
    from ._args import resolve_device
    inject = _resolve_inject(inject, fb)
    dev = resolve_device(device)
    if not plan.steps:
        return []
    mask = _checked_mask(mask, fb.nchans)
    setup = _plan_setup(fb, plan, gulp, kdm, zero_dm, block_mask)
    layout, table, nbits = setup["layout"], setup["table"], setup["nbits"]
    gulp, need_in, overlap, ws_bytes, off = (setup[k] for k in ("gulp", "need_in", "overlap", "ws_bytes", "out_floats"))
    if setup["total"] > int(budget_bytes):
        raise ValueError(f"dedispersing {len(plan)} DMs needs {setup['total']} bytes of device memory ({off * 4} of "
                         f"output plus the gulp buffers), over the budget of {int(budget_bytes)}: pass fewer DMs per "
                         "call (plan_slices)")
    with torch.cuda.device(dev):
        d_delays = torch.from_numpy(np.concatenate([d for d, _, _ in layout]).astype(np.int32)).to(dev)
        d_mask = None if mask is None else torch.from_numpy(mask).to(dev)
        workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        out = torch.empty(off, dtype=torch.float32, device=dev)
        d_bm = _upload_block_mask(fb, block_mask, dev, need_in)

        def process(block, start):
            # start is a multiple of every f: step k's outputs of this gulp begin at decimated sample start / f.
            # A short last gulp may hold no new output of a step (its rows are all inside the overlap)
            if inject is not None:
                engine.inject_device(block, inject[0], start, inject[1])
            steps = table.copy()
            steps["out_offset"] = start // steps["downsamp"]
            live = block.shape[0] // steps["downsamp"].astype(np.int64) > steps["max_delay"]
            if live.any():
                engine.dedisperse_steps_device(block, d_delays, steps[live], out, d_mask, workspace, None, zero_dm,
                                               nbits, d_bm, start)

        stream_gulps(fb, dev, gulp, need_in, overlap, process)
    return [out.as_strided((int(t["ndm"]), nout), (int(t["out_stride"]), 1), int(t["out_off"]))
            for t, (_, _, nout) in zip(table, layout)]
