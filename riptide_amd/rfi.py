"""RFI mitigation in front of the dedispersion of a filterbank file, on the
GPU where the samples already are (kernels in csrc/dedisp_kernels.hip):

  channel_stats   per-channel mean and standard deviation over the file,
                  streamed through the gulp machinery of dedisperse_filterbank
  channel_mask    those statistics to a channel mask (host, numpy): a simple
                  robust clip, ready to pass as mask=
  zero_dm_series  the zero-DM time series, every time sample's mean over the
                  unmasked channels: what zero_dm=True subtracts (Eatough,
                  Keane & Lyne 2009), and a diagnostic in its own right

  block_stats     the same statistics per (block of time, channel)
  block_mask      those to a mask in time and frequency (host, numpy) for
                  interference that is narrow in frequency and intermittent in
                  time: a BlockMask, the block_mask= argument of
                  dedisperse_filterbank and the search calls, which replace
                  every flagged cell's samples by the channel's fill as the
                  block is read on the device
  apply_block_mask_host  that replacement on the host: its specification

The zero-DM filter itself is the zero_dm=True argument of
dedispersion.dedisperse* and of search_filterbank.
"""
import ctypes
import warnings

import numpy as np

from . import _lib
from .dedispersion import (DEFAULT_BUDGET_BYTES, DEFAULT_GULP_BYTES, _checked_mask, _checked_sample_type, _gulp_layout,
                           _host_block, _upload_block_mask, stream_gulps)

__all__ = ["ChannelStats", "channel_stats", "channel_mask", "zero_dm_series", "BlockStats", "BlockMask", "block_stats",
           "block_mask", "apply_block_mask_host"]


class ChannelStats:
    """Per-channel statistics over `nsamp` time samples: `sum` and `sumsq`
    (float64 [nchans]; exact integers for 8-bit data), and derived from them
    on the host `mean` = sum / nsamp and `std` = sqrt(max(sumsq / nsamp -
    mean^2, 0))."""

    def __init__(self, sum, sumsq, nsamp):
        self.sum = np.asarray(sum, dtype=np.float64)
        self.sumsq = np.asarray(sumsq, dtype=np.float64)
        self.nsamp = int(nsamp)
        self.mean = self.sum / self.nsamp
        self.std = np.sqrt(np.clip(self.sumsq / self.nsamp - self.mean ** 2, 0.0, None))

    def __repr__(self):
        return f"ChannelStats(nchans={self.sum.size}, nsamp={self.nsamp})"


def _device_and_rows(fb, nsamp, gulp, device):
    from ._args import resolve_device
    dev = resolve_device(device)
    _checked_sample_type(fb)
    row_elems, dtype = _gulp_layout(fb)
    nrows = fb.nsamp if nsamp is None else int(nsamp)
    if not 0 < nrows <= fb.nsamp:
        raise ValueError(f"nsamp must be in [1, {fb.nsamp}]")
    if gulp is None:
        gulp = max(DEFAULT_GULP_BYTES // (row_elems * dtype.itemsize), 1)
    gulp = int(gulp)
    if gulp < 1:
        raise ValueError("gulp must be at least 1")
    return dev, nrows, min(gulp, nrows)


def channel_stats(fb, nsamp=None, gulp=None, device=None):
    """ChannelStats of a reading.Filterbank or PackedFilterbank, or of its first `nsamp` time
    samples: the file is streamed to `device` in gulps of `gulp` time samples
    (default: about 256 MiB) as dedisperse_filterbank streams it, and every
    gulp is added into float64 accumulators on the device
    (engine.channel_stats_device).  8-bit sums are exact whatever the gulp;
    the same call gives the same bits twice.  Waits for the result."""
    import torch
    from . import engine
    dev, nrows, gulp = _device_and_rows(fb, nsamp, gulp, device)
    with torch.cuda.device(dev):
        acc = torch.zeros((2, fb.nchans), dtype=torch.float64, device=dev)
        workspace = torch.empty(max(engine.channel_stats_workspace_bytes(gulp, fb.nchans), 16), dtype=torch.uint8,
                                device=dev)
        stream_gulps(fb, dev, gulp, nrows, 0,
                     lambda block, start: engine.channel_stats_device(block, acc, workspace=workspace,
                                                                      nbits=getattr(fb, "nbits", None)))
        host = acc.cpu().numpy()
    return ChannelStats(host[0], host[1], nrows)


def zero_dm_series(fb, mask=None, nsamp=None, gulp=None, device=None, block_mask=None):
    """The zero-DM time series of a reading.Filterbank or PackedFilterbank (or of its first
    `nsamp` time samples) as a float32 [nsamp] device tensor: every time
    sample's mean over the channels `mask` leaves (engine.zero_dm_mean_device
    per gulp).  block_mask (a BlockMask): the series of the file with the
    flagged cells replaced by their fill, what zero_dm=True subtracts when the
    same block mask is passed to the dedispersion call.  Queued on the current
    stream of `device`."""
    import torch
    from . import engine
    dev, nrows, gulp = _device_and_rows(fb, nsamp, gulp, device)
    mask = _checked_mask(mask, fb.nchans)
    with torch.cuda.device(dev):
        out = torch.empty(nrows, dtype=torch.float32, device=dev)
        d_mask = None if mask is None else torch.from_numpy(mask).to(dev)
        d_bm = _upload_block_mask(fb, block_mask, dev, nrows)
        stream_gulps(fb, dev, gulp, nrows, 0,
                     lambda block, start: engine.zero_dm_mean_device(block, mask=d_mask,
                                                                     out=out[start:start + block.shape[0]],
                                                                     nbits=getattr(fb, "nbits", None),
                                                                     block_mask=d_bm, t_origin=start))
    return out


class BlockStats:
    """Statistics per (block of `block_len` time samples, channel) over `nsamp`
    time samples: `sum` and `sumsq` (float64 [nblocks, nchans]; exact integers
    for integer data), `count` (int64 [nblocks], the samples of each block:
    block_len, but for a partial last block), and derived from them on the
    host `mean` = sum / count and `std` = sqrt(max(sumsq / count - mean^2, 0))."""

    def __init__(self, sum, sumsq, block_len, nsamp):
        self.sum = np.asarray(sum, dtype=np.float64)
        self.sumsq = np.asarray(sumsq, dtype=np.float64)
        self.block_len, self.nsamp = int(block_len), int(nsamp)
        if self.block_len < 1 or self.nsamp < 1:
            raise ValueError("block_len and nsamp must be at least 1")
        nblocks = -(-self.nsamp // self.block_len)
        if self.sum.ndim != 2 or self.sum.shape != self.sumsq.shape or self.sum.shape[0] != nblocks:
            raise ValueError(f"sum and sumsq must be [{nblocks}, nchans]")
        self.count = np.full(nblocks, self.block_len, dtype=np.int64)
        self.count[-1] = self.nsamp - (nblocks - 1) * self.block_len
        n = self.count[:, None].astype(np.float64)
        self.mean = self.sum / n
        self.std = np.sqrt(np.clip(self.sumsq / n - self.mean ** 2, 0.0, None))

    def __repr__(self):
        return (f"BlockStats(nblocks={self.sum.shape[0]}, nchans={self.sum.shape[1]}, block_len={self.block_len}, "
                f"nsamp={self.nsamp})")


def block_stats(fb, block_len=2048, nsamp=None, gulp=None, device=None, budget_bytes=DEFAULT_BUDGET_BYTES):
    """BlockStats of a reading.Filterbank or PackedFilterbank, or of its first
    `nsamp` time samples, in blocks of `block_len` time samples: the file is
    streamed to `device` as channel_stats streams it, in gulps of `gulp` time
    samples rounded down to a multiple of block_len (at least one block), so
    every block lies in one gulp and the result does not depend on gulp
    (engine.block_stats_device per gulp).  Integer sums are exact; the same
    call gives the same bits twice.  ValueError when the float64 result plus
    the gulp buffers exceed budget_bytes: use longer blocks.  Waits for the
    result."""
    import torch
    from . import engine
    block_len = int(block_len)
    if block_len < 1:
        raise ValueError("block_len must be at least 1")
    dev, nrows, gulp = _device_and_rows(fb, nsamp, gulp, device)
    gulp = max(gulp // block_len, 1) * block_len
    nblocks = -(-nrows // block_len)
    row_elems, dtype = _gulp_layout(fb)
    ws_bytes = engine.block_stats_workspace_bytes(min(gulp, nrows), fb.nchans, block_len)
    out_bytes = nblocks * 2 * fb.nchans * 8
    total = out_bytes + 2 * min(gulp, nrows) * row_elems * dtype.itemsize + ws_bytes
    if total > int(budget_bytes):
        raise ValueError(f"the statistics of {nblocks} blocks need {total} bytes of device memory ({out_bytes} of "
                         f"output plus the gulp buffers), over the budget of {int(budget_bytes)}: use longer blocks")
    with torch.cuda.device(dev):
        out = torch.empty((nblocks, 2, fb.nchans), dtype=torch.float64, device=dev)
        workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)

        def process(block, start):
            b0 = start // block_len
            engine.block_stats_device(block, block_len, out=out[b0:b0 + -(-block.shape[0] // block_len)],
                                      workspace=workspace, nbits=getattr(fb, "nbits", None))

        stream_gulps(fb, dev, min(gulp, nrows), nrows, 0, process)
        host = out.cpu().numpy()
    return BlockStats(host[:, 0], host[:, 1], block_len, nrows)


def _sample_range(fb_or_dtype, nbits=None):
    """(numpy dtype of a fill, lowest, highest value; None, None for float32)
    of a filterbank's samples, or of a dtype with nbits."""
    if nbits is None and hasattr(fb_or_dtype, "nchans"):
        nbits = getattr(fb_or_dtype, "nbits", None)
        fb_or_dtype = fb_or_dtype.dtype
    if nbits is not None:
        nbits = int(nbits)
        if nbits not in (1, 2, 4, 16):
            raise ValueError("nbits must be 1, 2, 4 or 16")
        return (np.dtype(np.uint16) if nbits == 16 else np.dtype(np.uint8)), 0, (1 << nbits) - 1
    dtype = np.dtype(fb_or_dtype)
    if dtype == np.float32:
        return dtype, None, None
    if dtype.name not in ("uint8", "int8"):
        raise ValueError("the samples must be uint8, int8, float32, or packed with nbits 1, 2, 4 or 16")
    return dtype, int(np.iinfo(dtype).min), int(np.iinfo(dtype).max)


class BlockMask:
    """A mask in time and frequency: `cells` bool [nblocks, nchans], True =
    the channel is flagged during block b, the samples [b * block_len, (b + 1)
    * block_len) of the file; `fill` float64 [nchans], the value a flagged
    cell's samples are replaced by (typed_fill gives it in a file's sample
    type).  The block_mask= argument of dedisperse_filterbank, band_series,
    zero_dm_series, search_filterbank, search_filterbank_pulses and
    build_candidates_filterbank."""

    def __init__(self, cells, block_len, fill):
        self.cells = np.ascontiguousarray(np.asarray(cells).astype(bool))
        self.block_len = int(block_len)
        self.fill = np.ascontiguousarray(fill, dtype=np.float64)
        if self.block_len < 1:
            raise ValueError("block_len must be at least 1")
        if self.cells.ndim != 2 or self.fill.shape != (self.cells.shape[1],):
            raise ValueError("cells must be [nblocks, nchans] and fill [nchans]")

    @property
    def nblocks(self):
        return self.cells.shape[0]

    @property
    def nchans(self):
        return self.cells.shape[1]

    @property
    def fraction(self):
        """The flagged share of the cells."""
        return float(self.cells.mean()) if self.cells.size else 0.0

    def channel_mask(self):
        """bool [nchans]: the channels flagged in every block, to be or-ed
        into the mask= argument (a fully flagged channel would otherwise
        still add its constant fill to every sum)."""
        return self.cells.all(axis=0) if self.nblocks else np.zeros(self.nchans, dtype=bool)

    def typed_fill(self, fb, nbits=None):
        """fill in the sample type of `fb` (a Filterbank or PackedFilterbank;
        or a numpy dtype, with nbits for packed data), as the device and
        apply_block_mask_host take it: integer types rounded to nearest
        (numpy's rint) and clipped to the sample's range -- uint8 for uint8
        and 1/2/4-bit data, int8, uint16 for 16-bit data -- and a float32
        cast for float32."""
        dtype, lo, hi = _sample_range(fb, nbits)
        if lo is None:
            return self.fill.astype(np.float32)
        return np.clip(np.rint(self.fill), lo, hi).astype(dtype)

    def save(self, fname):
        """Write cells, block_len and fill to `fname` as a numpy .npz archive."""
        with open(fname, "wb") as f:
            np.savez(f, cells=self.cells, block_len=np.int64(self.block_len), fill=self.fill)

    @classmethod
    def load(cls, fname):
        with np.load(fname) as z:
            return cls(z["cells"], int(z["block_len"]), z["fill"])

    def __repr__(self):
        return (f"BlockMask(nblocks={self.nblocks}, nchans={self.nchans}, block_len={self.block_len}, "
                f"fraction={self.fraction:.4f})")


def block_mask(stats, threshold=4.0, max_iter=5, chan_frac=0.3, block_frac=0.3):
    """A BlockMask from BlockStats: channel_mask's robust clip turned to run
    along time, channel by channel.  Host numpy only.

    1. Cells of full blocks whose std is 0 (dead or stuck) are flagged.
    2. Then per channel, at most max_iter times and until nothing changes,
       cells of full blocks whose block mean or std lies more than threshold *
       1.4826 * MAD from the median are flagged, median and MAD taken over
       that channel's unflagged full blocks.
    3. A trailing partial block is not tested: it takes the flags of the block
       before it, if there is one.
    4. A channel whose flagged share of blocks exceeds chan_frac is flagged
       everywhere.
    5. A block whose flagged share of channels exceeds block_frac is flagged
       everywhere.

    fill[c] is the channel's mean over its unflagged full blocks, or over the
    whole file when it has none."""
    mean = np.asarray(stats.mean, dtype=np.float64)
    std = np.asarray(stats.std, dtype=np.float64)
    nblocks, nchans = mean.shape
    full = np.asarray(stats.count) == stats.block_len
    fmean, fstd = mean[full], std[full]
    flagged = fstd == 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # a channel with nothing left: all-NaN medians
        for _ in range(int(max_iter)):
            new = flagged.copy()
            for v in (fstd, fmean):
                good = np.where(flagged, np.nan, v)
                med = np.nanmedian(good, axis=0) if good.size else np.zeros(nchans)
                cut = float(threshold) * 1.4826 * (np.nanmedian(np.abs(good - med), axis=0) if good.size
                                                  else np.zeros(nchans))
                with np.errstate(invalid="ignore"):
                    new |= np.abs(v - med) > cut      # NaN median (nothing unflagged): False
            if np.array_equal(new, flagged):
                break
            flagged = new
    cells = np.zeros((nblocks, nchans), dtype=bool)
    cells[full] = flagged
    if nblocks and not full[-1] and nblocks > 1:
        cells[-1] = cells[-2]
    if nblocks:
        cells[:, cells.mean(axis=0) > float(chan_frac)] = True
        cells[cells.mean(axis=1) > float(block_frac), :] = True
    keep = ~cells & full[:, None]
    total = np.asarray(stats.sum, dtype=np.float64)
    n = keep.sum(axis=0) * float(stats.block_len)
    whole = total.sum(axis=0) / float(stats.nsamp) if stats.nsamp else np.zeros(nchans)
    with np.errstate(invalid="ignore", divide="ignore"):
        fill = np.where(n > 0, np.where(keep, total, 0.0).sum(axis=0) / n, whole)
    return BlockMask(cells, stats.block_len, fill)


def apply_block_mask_host(data, cells, block_len, fill, t_origin=0, nbits=None):
    """The replacement a block mask stands for, on the host
    (rt_block_replace_host, no device): a copy of `data` -- [nsamp, nchans]
    uint8, int8 or float32, or with nbits packed rows uint8 [nsamp, row_bytes]
    -- in which every sample (t, c) with cells[(t_origin + t) // block_len, c]
    set is fill[c].  `fill` is [nchans] in the sample's own type
    (BlockMask.typed_fill): the data's dtype, uint8 for 1/2/4-bit data (the low
    nbits bits are used), uint16 for 16-bit data.  ValueError when the rows
    reach past the cells or the fill has another dtype."""
    data, code, nsamp, nchans = _host_block(data, nbits)
    cells = np.ascontiguousarray(np.asarray(cells).astype(bool), dtype=np.uint8)
    if cells.ndim != 2 or cells.shape[1] != nchans:
        raise ValueError(f"cells must be [nblocks, {nchans}]")
    want, _, _ = _sample_range(data.dtype, nbits)
    fill = np.asarray(fill)
    if fill.dtype != want or fill.shape != (nchans,):
        raise ValueError(f"fill must be a {want.name} array [{nchans}]: one value per channel in the sample's own type")
    fill = np.ascontiguousarray(fill)
    if not 0 <= int(t_origin) < 1 << 64 or int(block_len) < 1:
        raise ValueError("block_len must be at least 1 and t_origin in [0, 2^64)")
    out = np.empty_like(data)
    bm = _lib.BlockMaskStruct(cells.ctypes.data, cells.shape[0], int(block_len), int(t_origin), fill.ctypes.data)
    _lib.check(_lib.load().rt_block_replace_host(_lib.ptr(data), code, nsamp, nchans, ctypes.byref(bm), _lib.ptr(out)))
    return out


def channel_mask(stats, threshold=4.0, max_iter=5):
    """A channel mask (bool [nchans], True = skip: the mask= argument of the
    dedispersion calls) from ChannelStats.  A simple robust clip, not a
    replacement for a full RFI package:

    - channels whose std is 0 (dead or stuck) are flagged;
    - then, at most max_iter times and until nothing changes, channels whose
      std or mean lies more than threshold * 1.4826 * MAD from the median are
      flagged, median and MAD (median absolute deviation; 1.4826 MAD estimates
      a normal distribution's sigma) taken over the channels not yet flagged.

    A band whose unflagged channels are all equal has MAD 0 and flags nothing
    further.  Host numpy only."""
    std = np.asarray(stats.std, dtype=np.float64)
    mean = np.asarray(stats.mean, dtype=np.float64)
    flagged = std == 0.0
    for _ in range(int(max_iter)):
        good = ~flagged
        if not good.any():
            break
        new = flagged.copy()
        for v in (std, mean):
            med = np.median(v[good])
            cut = float(threshold) * 1.4826 * np.median(np.abs(v[good] - med))
            new |= np.abs(v - med) > cut
        if np.array_equal(new, flagged):
            break
        flagged = new
    return flagged
