"""RFI mitigation in front of the dedispersion of a filterbank file, on the
GPU where the samples already are (kernels in csrc/dedisp_kernels.hip):

  channel_stats   per-channel mean and standard deviation over the file,
                  streamed through the gulp machinery of dedisperse_filterbank
  channel_mask    those statistics to a channel mask (host, numpy): a simple
                  robust clip, ready to pass as mask=
  zero_dm_series  the zero-DM time series, every time sample's mean over the
                  unmasked channels: what zero_dm=True subtracts (Eatough,
                  Keane & Lyne 2009), and a diagnostic in its own right

The zero-DM filter itself is the zero_dm=True argument of
dedispersion.dedisperse* and of search_filterbank.
"""
import numpy as np

from .dedispersion import DEFAULT_GULP_BYTES, _checked_mask, _checked_sample_type, _gulp_layout, stream_gulps

__all__ = ["ChannelStats", "channel_stats", "channel_mask", "zero_dm_series"]


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
    import torch
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else
                       (device.index if isinstance(device, torch.device) else int(device)))
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


def zero_dm_series(fb, mask=None, nsamp=None, gulp=None, device=None):
    """The zero-DM time series of a reading.Filterbank or PackedFilterbank (or of its first
    `nsamp` time samples) as a float32 [nsamp] device tensor: every time
    sample's mean over the channels `mask` leaves (engine.zero_dm_mean_device
    per gulp).  Queued on the current stream of `device`."""
    import torch
    from . import engine
    dev, nrows, gulp = _device_and_rows(fb, nsamp, gulp, device)
    mask = _checked_mask(mask, fb.nchans)
    with torch.cuda.device(dev):
        out = torch.empty(nrows, dtype=torch.float32, device=dev)
        d_mask = None if mask is None else torch.from_numpy(mask).to(dev)
        stream_gulps(fb, dev, gulp, nrows, 0,
                     lambda block, start: engine.zero_dm_mean_device(block, mask=d_mask,
                                                                     out=out[start:start + block.shape[0]],
                                                                     nbits=getattr(fb, "nbits", None)))
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
