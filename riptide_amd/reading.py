"""Readers of dedispersed time series files: SIGPROC .tim and PRESTO .inf/.dat
(riptide/reading/sigproc.py:1-197, riptide/reading/presto.py:1-149,
riptide/metadata.py:54-106, riptide/time_series.py:283-362).

Header parsing stays on the host; the bulk samples are read as raw bytes and,
for the device path (`load_device_batch`), converted to float32 on the GPU by
rt_convert_samples_device after one host-to-device copy of the raw bytes
(8-bit data moves 4x fewer bytes over PCIe than its float32 expansion).

astropy is not available here: sky coordinates are kept as `Coord`
(right ascension in hours, declination in degrees), parsed exactly as the
reference parses them before building its SkyCoord.
"""
import os
import struct
import typing

import numpy as np

from .metadata import Metadata


class Coord(typing.NamedTuple):
    """ICRS position: right ascension (hours), declination (degrees)."""
    ra_hours: float
    dec_deg: float


# ---------------------------------------------------------------------------
# SIGPROC (riptide/reading/sigproc.py)
# ---------------------------------------------------------------------------
# Header keys and their stored types: int = int32, float = float64,
# bool = unsigned char, str = int32 length + bytes (sigproc.py:18-62).
SIGPROC_KEYS = {
    "filename": str, "telescope_id": int, "telescope": str, "machine_id": int, "data_type": int,
    "rawdatafile": str, "source_name": str, "barycentric": int, "pulsarcentric": int, "az_start": float,
    "za_start": float, "src_raj": float, "src_dej": float, "tstart": float, "tsamp": float, "nbits": int,
    "nsamples": int, "fch1": float, "foff": float, "fchannel": float, "nchans": int, "nifs": int,
    "refdm": float, "flux": float, "period": float, "nbeams": int, "ibeam": int, "hdrlen": int, "pb": float,
    "ecc": float, "asini": float, "orig_hdrlen": int, "new_hdrlen": int, "sampsize": int, "bandwidth": float,
    "fbottom": float, "ftop": float, "obs_date": str, "obs_time": str, "accel": float, "signed": bool,
}
HEADER_START = "HEADER_START"
HEADER_END = "HEADER_END"


def _read_str(f):
    (size,) = struct.unpack("i", f.read(4))
    return f.read(size).decode()


def read_sigproc_header(f, extra_keys=None):
    """({key: value}, header byte size) of an open SIGPROC file (sigproc.py:109-147)."""
    keys = dict(SIGPROC_KEYS)
    if extra_keys:
        keys.update(extra_keys)
    f.seek(0)
    flag = _read_str(f)
    assert flag == HEADER_START, f"File starts with {flag!r} flag instead of the expected {HEADER_START!r}"
    attrs = {}
    while True:
        key = _read_str(f)
        if key == HEADER_END:
            break
        atype = keys.get(key)
        if atype is None:
            raise KeyError(f"Type of SIGPROC header attribute {key!r} is unknown, please specify it")
        if atype is str:
            val = _read_str(f)
        elif atype is int:
            (val,) = struct.unpack("i", f.read(4))
        elif atype is float:
            (val,) = struct.unpack("d", f.read(8))
        elif atype is bool:
            (val,) = struct.unpack("B", f.read(1))
            val = bool(val)
        else:
            raise ValueError(f"Key {key!r} has unsupported type {atype!r}")
        attrs[key] = val
    return attrs, f.tell()


def parse_float_coord(x):
    """SIGPROC's ddmmss.s / hhmmss.s float coordinate -> hours or degrees (sigproc.py:150-159)."""
    sign = np.sign(x)
    x = abs(x)
    hh, x = divmod(x, 10000.0)
    mm, ss = divmod(x, 100.0)
    return sign * (hh + mm / 60.0 + ss / 3600.0)


class SigprocHeader(dict):
    """Header of a SIGPROC file (sigproc.py:159-197)."""

    def __init__(self, fname, extra_keys=None):
        self._fname = os.path.abspath(fname)
        with open(self._fname, "rb") as f:
            attrs, self._bytesize = read_sigproc_header(f, extra_keys)
        super().__init__(attrs)

    @property
    def fname(self):
        return self._fname

    @property
    def bytesize(self):
        return self._bytesize

    @property
    def bytes_per_sample(self):
        return self["nchans"] * self["nbits"] // 8

    @property
    def nsamp(self):
        return (os.path.getsize(self.fname) - self.bytesize) // self.bytes_per_sample

    @property
    def tobs(self):
        return self.nsamp * self["tsamp"]

    @property
    def skycoord(self):
        return Coord(float(parse_float_coord(self["src_raj"])), float(parse_float_coord(self["src_dej"])))


def sigproc_metadata(sh):
    """Metadata.from_sigproc (metadata.py:74-106): checks and derived keys."""
    if sh["nchans"] > 1:
        raise ValueError(f"File {sh.fname!r} contains multi-channel data (nchans = {sh['nchans']}), "
                         "instead of a dedispersed time series")
    nbits = sh["nbits"]
    if nbits not in {8, 32}:
        raise ValueError(f"Only 8-bit and 32-bit SIGPROC data are supported. File {sh.fname!r} contains "
                         f"{nbits}-bit data")
    if nbits == 8 and "signed" not in sh:
        raise ValueError("SIGPROC Header says this is 8-bit data, but does not specify its signedness via the "
                         "'signed' key")
    attrs = dict(sh)
    attrs["dm"] = attrs.get("refdm", None)
    attrs["skycoord"] = sh.skycoord
    attrs["source_name"] = attrs.get("source_name", None)
    attrs["mjd"] = attrs.get("tstart", None)
    attrs["fname"] = os.path.realpath(sh.fname)
    attrs["tobs"] = sh.tobs
    return Metadata(attrs)


def sigproc_sample_dtype(meta):
    if meta["nbits"] == 8:
        return np.int8 if meta["signed"] else np.uint8
    return np.float32


def read_sigproc(fname, extra_keys=None):
    """(float32 samples, Metadata, tsamp) as TimeSeries.from_sigproc (time_series.py:320-362)."""
    sh = SigprocHeader(fname, extra_keys=extra_keys)
    meta = sigproc_metadata(sh)
    with open(sh.fname, "rb") as f:
        f.seek(sh.bytesize)
        data = np.fromfile(f, dtype=sigproc_sample_dtype(meta)).astype(np.float32)
    return data, meta, sh["tsamp"]


class Filterbank:
    """A channelised SIGPROC file (nchans >= 1, one IF), opened for
    dedispersion: the samples are a read-only memory map, nothing is read
    until a slice of it is taken.

      header   the SigprocHeader
      nsamp, nchans, tsamp
      freqs    channel centre frequencies in MHz, fch1 + c * foff (foff of
               either sign), float64 [nchans]
      dtype    sample type: 8-bit data is unsigned unless the header key
               `signed` says otherwise; 32-bit data is float
      data     np.memmap [nsamp, nchans], time-major as stored

    1-, 2-, 4- and 16-bit data is refused here: open_filterbank opens any of
    the six widths (those four as a PackedFilterbank)."""

    def __init__(self, fname, extra_keys=None):
        sh = SigprocHeader(fname, extra_keys=extra_keys)
        if sh.get("nifs", 1) != 1:
            raise ValueError(f"File {sh.fname!r} has nifs = {sh['nifs']}; only single-IF filterbanks are supported")
        nbits = sh["nbits"]
        if nbits not in {8, 32}:
            raise ValueError(f"Only 8-bit and 32-bit SIGPROC data are supported. File {sh.fname!r} contains "
                             f"{nbits}-bit data")
        self._set_shape(sh)
        if nbits == 32:
            self.dtype = np.dtype(np.float32)
        else:
            self.dtype = np.dtype(np.int8 if sh.get("signed", False) else np.uint8)
        self.data = np.memmap(sh.fname, dtype=self.dtype, mode="r", offset=sh.bytesize,
                              shape=(self.nsamp, self.nchans))

    def _set_shape(self, sh):
        """header, fname, nchans, tsamp, nsamp and freqs from the header."""
        self.header = sh
        self.fname = sh.fname
        self.nchans = int(sh["nchans"])
        if self.nchans < 1:
            raise ValueError(f"File {sh.fname!r} has nchans = {self.nchans}")
        if self.nchans * int(sh["nbits"]) % 8:
            raise ValueError(f"File {sh.fname!r} has {self.nchans} channels of {sh['nbits']}-bit data: rows are not "
                             "a whole number of bytes")
        self.tsamp = float(sh["tsamp"])
        self.nsamp = int(sh.nsamp)
        if self.nsamp < 1:
            raise ValueError(f"File {sh.fname!r} holds no samples")
        self.freqs = float(sh["fch1"]) + np.arange(self.nchans, dtype=np.float64) * float(sh["foff"])

    @property
    def tobs(self):
        return self.nsamp * self.tsamp

    def metadata(self, dm=None):
        """The file's header as the Metadata of a series dedispersed at `dm`
        (the keys sigproc_metadata derives, without its single-channel check)."""
        sh = self.header
        attrs = dict(sh)
        attrs["dm"] = dm
        attrs["skycoord"] = sh.skycoord if "src_raj" in sh and "src_dej" in sh else None
        attrs["source_name"] = attrs.get("source_name", None)
        attrs["mjd"] = attrs.get("tstart", None)
        attrs["fname"] = os.path.realpath(sh.fname)
        attrs["tobs"] = self.tobs
        return Metadata(attrs)


PACKED_NBITS = (1, 2, 4, 16)


def _packed_row_bytes(nbits, nchans):
    nbits, nchans = int(nbits), int(nchans)
    if nbits not in PACKED_NBITS:
        raise ValueError(f"nbits must be one of {PACKED_NBITS}, not {nbits}")
    if nchans < 1 or nchans * nbits % 8:
        raise ValueError(f"{nchans} channels of {nbits}-bit data: rows are not a whole number of bytes")
    return nchans * nbits // 8


def unpack_samples(raw, nbits, nchans):
    """Packed rows -> sample values [n, nchans], uint8 for 1-, 2- and 4-bit
    data and uint16 for 16-bit data (host numpy).  `raw` is uint8, [n,
    row_bytes] or flat, row_bytes = nchans * nbits / 8.  The format, for host
    and device alike (include/riptide_amd.h):

      1, 2, 4 bit  unsigned, SIGPROC's packing, least significant bits first:
                   (row[(c * nbits) >> 3] >> ((c * nbits) & 7)) & (2^nbits - 1)
      16 bit       unsigned, little-endian: row[2c] | row[2c + 1] << 8

    A most-significant-bit-first packing is not supported."""
    rb = _packed_row_bytes(nbits, nchans)
    raw = np.asarray(raw)
    if raw.dtype != np.uint8 or raw.size % rb:
        raise ValueError(f"raw must be uint8 rows of {rb} bytes")
    raw = raw.reshape(-1, rb)
    if nbits == 16:
        return (raw[:, 0::2].astype(np.uint16) | (raw[:, 1::2].astype(np.uint16) << 8))
    bit = np.arange(nchans) * nbits
    return np.ascontiguousarray((raw[:, bit >> 3] >> (bit & 7).astype(np.uint8)) & np.uint8((1 << nbits) - 1))


def pack_samples(x, nbits):
    """Integer samples [n, nchans], each in [0, 2^nbits), -> packed rows uint8
    [n, nchans * nbits / 8], the inverse of unpack_samples (host numpy).
    ValueError for a value out of range and for rows that are not a whole
    number of bytes."""
    x = np.asarray(x)
    if x.ndim != 2 or x.dtype.kind not in "iub":
        raise ValueError("x must be an integer array [n, nchans]")
    rb = _packed_row_bytes(nbits, x.shape[1])
    if x.size and (int(x.min()) < 0 or int(x.max()) >= 1 << nbits):
        raise ValueError(f"samples must be in [0, {1 << nbits}) for {nbits}-bit data")
    if nbits == 16:
        out = np.empty((x.shape[0], rb), dtype=np.uint8)
        out[:, 0::2] = x & 0xFF
        out[:, 1::2] = x >> 8
        return out
    per = 8 // nbits
    fields = x.astype(np.uint8).reshape(x.shape[0], rb, per) << (np.arange(per) * nbits).astype(np.uint8)
    return np.bitwise_or.reduce(fields, axis=2)


class PackedFilterbank(Filterbank):
    """A channelised SIGPROC file of 1-, 2-, 4- or 16-bit samples (the format:
    unpack_samples), opened for dedispersion as a Filterbank is.  The rows stay
    packed up to the device, which unpacks them inside its transpose.

      nbits      1, 2, 4 or 16
      row_bytes  nchans * nbits / 8 (a whole number: ValueError otherwise)
      dtype      type of the unpacked values: uint8, or uint16 for 16 bit
      data       read-only np.memmap of the raw rows, uint8 [nsamp, row_bytes]
      unpack(start=0, stop=None)   unpack_samples of those rows

    The samples are unsigned: a `signed` header key is ignored for 1-, 2- and
    4-bit data and refused (ValueError) for 16-bit data.  header, nsamp,
    nchans, tsamp, freqs, tobs and metadata() are the base class's."""

    def __init__(self, fname, extra_keys=None):
        sh = SigprocHeader(fname, extra_keys=extra_keys)
        if sh.get("nifs", 1) != 1:
            raise ValueError(f"File {sh.fname!r} has nifs = {sh['nifs']}; only single-IF filterbanks are supported")
        nbits = int(sh["nbits"])
        if nbits not in PACKED_NBITS:
            raise ValueError(f"File {sh.fname!r} contains {nbits}-bit data, not 1-, 2-, 4- or 16-bit packed data")
        if nbits == 16 and sh.get("signed", False):
            raise ValueError(f"File {sh.fname!r} holds signed 16-bit data; only unsigned 16-bit data is supported")
        self._set_shape(sh)
        self.nbits = nbits
        self.row_bytes = self.nchans * nbits // 8
        self.dtype = np.dtype(np.uint16 if nbits == 16 else np.uint8)
        self.data = np.memmap(sh.fname, dtype=np.uint8, mode="r", offset=sh.bytesize,
                              shape=(self.nsamp, self.row_bytes))

    def unpack(self, start=0, stop=None):
        """The values of rows [start, stop) as [n, nchans] of `dtype`."""
        return unpack_samples(np.asarray(self.data[start:stop]), self.nbits, self.nchans)


def open_filterbank(fname, extra_keys=None):
    """Open a channelised SIGPROC file of any supported width: a Filterbank
    for 8- and 32-bit data, a PackedFilterbank for 1-, 2-, 4- and 16-bit
    data.  Any other width is refused as Filterbank refuses it."""
    with open(fname, "rb") as f:
        attrs, _ = read_sigproc_header(f, extra_keys)
    if attrs.get("nbits") in PACKED_NBITS:
        return PackedFilterbank(fname, extra_keys=extra_keys)
    return Filterbank(fname, extra_keys=extra_keys)


def write_sigproc(fname, data, header):
    """Write a SIGPROC file (used by tests and tools; the header keys must be
    in SIGPROC_KEYS): a time series from 1-D data, or a filterbank from data
    [nsamp, nchans], written time-major as given (the header's nchans must
    then equal the second dimension, and the array's item size its nbits)."""
    data = np.asarray(data)
    if data.ndim == 2:
        if int(header.get("nchans", -1)) != data.shape[1]:
            raise ValueError("write_sigproc: header nchans must equal the channels of 2-D data")
        if int(header.get("nbits", -1)) != 8 * data.dtype.itemsize:
            raise ValueError("write_sigproc: header nbits must equal the bits of a 2-D array's samples")
    elif data.ndim > 2:
        raise ValueError("write_sigproc: data must be 1-D or [nsamp, nchans]")

    def wstr(f, s):
        b = s.encode()
        f.write(struct.pack("i", len(b)))
        f.write(b)

    with open(fname, "wb") as f:
        wstr(f, HEADER_START)
        for key, val in header.items():
            wstr(f, key)
            t = SIGPROC_KEYS[key]
            if t is str:
                wstr(f, val)
            elif t is int:
                f.write(struct.pack("i", int(val)))
            elif t is float:
                f.write(struct.pack("d", float(val)))
            elif t is bool:
                f.write(struct.pack("B", int(bool(val))))
        wstr(f, HEADER_END)
        np.ascontiguousarray(data).tofile(f)


# ---------------------------------------------------------------------------
# PRESTO (riptide/reading/presto.py)
# ---------------------------------------------------------------------------
SEP_COLUMN = 40
FAKE_TELESCOPE = "None (Artificial Data Set)"


def _inf_value(line, vtype):
    if not (len(line) > SEP_COLUMN and line[SEP_COLUMN] == "="):
        raise ValueError(f"Expected '=' character at column {SEP_COLUMN}")
    return vtype(line[SEP_COLUMN + 1:].strip())


def _bool01(s):
    return int(s) != 0


def _int_pair(s):
    a, b = s.split(",")
    return int(a), int(b)


def inf2dict(text):
    """Parse the text of a PRESTO .inf file (presto.py:55-125)."""
    lines = text.strip("\n").splitlines()

    def p(n, vtype):
        return _inf_value(lines[n], vtype)

    basename, telescope = p(0, str), p(1, str)
    if telescope == FAKE_TELESCOPE:
        raise ValueError("Reading data generated with PRESTO's makedata is not supported")
    items = {"basename": basename, "telescope": telescope, "instrument": p(2, str), "source_name": p(3, str),
             "raj": p(4, str), "decj": p(5, str), "observer": p(6, str), "mjd": p(7, float),
             "barycentered": p(8, _bool01), "nsamp": p(9, int), "tsamp": p(10, float), "breaks": p(11, _bool01),
             "onoff_pairs": []}
    lines = lines[12:]
    if items["breaks"]:
        for line in lines:
            try:
                items["onoff_pairs"].append(_inf_value(line, _int_pair))
            except Exception:
                break
    lines = lines[len(items["onoff_pairs"]):]
    em_band = p(0, str)
    items["em_band"] = em_band
    if em_band == "Radio":
        for k, (key, t) in enumerate([("fov_arcsec", float), ("dm", float), ("fbot", float), ("bandwidth", float),
                                      ("nchan", int), ("cbw", float), ("analyst", str)], start=1):
            items[key] = p(k, t)
    elif em_band in ("X-ray", "Gamma"):
        for k, (key, t) in enumerate([("fov_arcsec", float), ("central_energy_kev", float),
                                      ("energy_bandpass_kev", float), ("analyst", str)], start=1):
            items[key] = p(k, t)
    else:
        raise ValueError(f"EM Band {em_band!r} not supported")
    return items


def _sexagesimal(s):
    sign = -1.0 if s.strip().startswith("-") else 1.0
    parts = [abs(float(x)) for x in s.strip().lstrip("+-").split(":")]
    while len(parts) < 3:
        parts.append(0.0)
    return sign * (parts[0] + parts[1] / 60.0 + parts[2] / 3600.0)


class PrestoInf(dict):
    """PRESTO .inf metadata (presto.py:124-149)."""

    def __init__(self, fname):
        self._fname = os.path.realpath(fname)
        with open(fname, "r") as f:
            items = inf2dict(f.read())
        super().__init__(items)

    @property
    def fname(self):
        return self._fname

    @property
    def data_fname(self):
        return self.fname.rsplit(".", maxsplit=1)[0] + ".dat"

    @property
    def skycoord(self):
        return Coord(_sexagesimal(self["raj"]), _sexagesimal(self["decj"]))

    def load_data(self):
        return np.fromfile(self.data_fname, dtype=np.float32)


def presto_metadata(inf):
    """Metadata.from_presto_inf (metadata.py:54-71)."""
    attrs = dict(inf)
    attrs["skycoord"] = inf.skycoord
    attrs["fname"] = os.path.realpath(inf.fname)
    attrs["tobs"] = attrs["tsamp"] * attrs["nsamp"]
    return Metadata(attrs)


def read_presto(fname):
    """(float32 samples, Metadata, tsamp) as TimeSeries.from_presto_inf (time_series.py:283-318)."""
    inf = PrestoInf(fname)
    meta = presto_metadata(inf)
    if meta["em_band"] in ("X-ray", "Gamma"):
        import warnings
        warnings.warn(f" You have loaded file {fname!r}, which contains data observed at a high-energy band "
                      f"{meta['em_band']!r}. riptide is NOT designed to process low photon count time series, "
                      "i.e. where the background noise statistics are non-Gaussian. Be VERY careful when "
                      "interpreting any search outputs.", category=UserWarning)
    return inf.load_data(), meta, inf["tsamp"]


# ---------------------------------------------------------------------------
# Device batch loading
# ---------------------------------------------------------------------------
def _raw_samples(fname, fmt, extra_keys=None, staging=None):
    """(raw numpy samples as stored, Metadata, tsamp) without the float cast.
    `staging(nbytes)`, if given, returns a writable uint8 numpy array of at
    least nbytes (page-locked host memory) that SIGPROC samples are read into
    directly; the samples returned are then a view of it."""
    if fmt == "sigproc":
        sh = SigprocHeader(fname, extra_keys=extra_keys)
        meta = sigproc_metadata(sh)
        dt = np.dtype(sigproc_sample_dtype(meta))
        with open(sh.fname, "rb") as f:
            f.seek(sh.bytesize)
            if staging is None:
                raw = np.fromfile(f, dtype=dt)
            else:
                nbytes = (os.path.getsize(sh.fname) - sh.bytesize) // dt.itemsize * dt.itemsize
                buf = staging(nbytes)[:nbytes]
                got = f.readinto(memoryview(buf))
                if got != nbytes:
                    raise OSError(f"short read from {sh.fname}: {got} of {nbytes} bytes")
                raw = buf.view(dt)
        return raw, meta, sh["tsamp"]
    if fmt == "presto":
        data, meta, tsamp = read_presto(fname)
        return data, meta, tsamp
    raise ValueError(f"unknown time series format {fmt!r}")


def upload_samples(raws, device=None, stream=None):
    """Host sample arrays of equal length (float32, or uint8 / int8 8-bit data
    as stored) -> one float32 [B, N] device tensor.  8-bit samples are copied
    to the device as bytes (4x fewer bytes over PCIe than their float32
    expansion) and converted there by rt_convert_samples_device, bit-exact
    with numpy's astype(float32)."""
    import torch
    from . import _lib
    from ._args import resolve_device, stream_scope
    dev = resolve_device(device)
    n = int(raws[0].size)
    if any(int(r.size) != n for r in raws):
        raise ValueError("upload_samples needs series of equal length")
    L = _lib.load()
    kinds = {np.dtype(np.uint8): 0, np.dtype(np.int8): 1}
    with stream_scope(dev, stream) as (_, handle):
        out = torch.empty((len(raws), n), dtype=torch.float32, device=dev)
        for b, raw in enumerate(raws):
            raw = np.asarray(raw)
            if raw.dtype != np.float32 and raw.dtype not in kinds:
                raw = raw.astype(np.float32)      # e.g. float64 series (EngineSearcher's old cast)
            raw = np.ascontiguousarray(raw)
            src = torch.from_numpy(raw if raw.dtype == np.float32 else raw.view(np.uint8))
            # asynchronous only from page-locked memory (_raw_samples' staging
            # slots, whose owner waits for the stream before refilling them);
            # pageable sources (and temporaries made here) are copied
            # synchronously, so nothing dropped below is still being read
            pinned = src.is_pinned()
            if raw.dtype == np.float32:
                out[b].copy_(src, non_blocking=pinned)
                continue
            staged = src.to(dev, non_blocking=pinned)
            _lib.check(L.rt_convert_samples_device(_lib.ptr(staged), n, kinds[raw.dtype], _lib.ptr(out[b]), handle))
    return out


def load_device_batch(fnames, fmt="sigproc", device=None, extra_keys=None, stream=None):
    """Load time series files of equal length into one float32 [B, N] device
    tensor (upload_samples).  Returns (tensor, [Metadata], tsamp)."""
    raws, metas, tsamps = [], [], []
    for fn in fnames:
        raw, meta, tsamp = _raw_samples(fn, fmt, extra_keys)
        raws.append(raw)
        metas.append(meta)
        tsamps.append(tsamp)
    if any(t != tsamps[0] for t in tsamps):
        raise ValueError("load_device_batch needs files of equal length and sampling time")
    return upload_samples(raws, device=device, stream=stream), metas, tsamps[0]


def write_presto(basename, data, tsamp, dm=0.0, mjd=60000.0, em_band="Radio"):
    """Write a PRESTO .inf/.dat pair (float32 samples; used by tests, tools and
    the cfg5 bench leg).  The .inf carries the keys inf2dict reads, one per
    line, value after '=' at column 40, as PRESTO's own writer lays them out."""
    data = np.ascontiguousarray(data, dtype=np.float32)
    name = os.path.basename(basename)

    def line(label, value):
        return f" {label:<39s}=  {value}"

    rows = [line("Data file name without suffix", name),
            line("Telescope used", "Parkes"),
            line("Instrument used", "Multibeam"),
            line("Object being observed", "Fake"),
            line("J2000 Right Ascension (hh:mm:ss.ssss)", "00:00:01.0000"),
            line("J2000 Declination     (dd:mm:ss.ssss)", "-00:00:01.0000"),
            line("Data observed by", "riptide_amd"),
            line("Epoch of observation (MJD)", f"{mjd:.6f}"),
            line("Barycentered?           (1=yes, 0=no)", "1"),
            line("Number of bins in the time series", f"{data.size:d}"),
            line("Width of each time series bin (sec)", f"{tsamp:.12e}"),
            line("Any breaks in the data? (1=yes, 0=no)", "0"),
            line("Type of observation (EM band)", em_band)]
    if em_band == "Radio":
        rows += [line("Beam diameter (arcsec)", "981"),
                 line("Dispersion measure (cm-3 pc)", f"{dm:.12f}"),
                 line("Central freq of low channel (Mhz)", "1182.1953125"),
                 line("Total bandwidth (Mhz)", "400"),
                 line("Number of channels", "1024"),
                 line("Channel bandwidth (Mhz)", "0.390625"),
                 line("Data analyzed by", "riptide_amd")]
    else:
        rows += [line("Field-of-view diameter (arcsec)", "100"),
                 line("Central energy (kev)", "1.0"),
                 line("Energy bandpass (kev)", "1.0"),
                 line("Data analyzed by", "riptide_amd")]
    with open(basename + ".inf", "w") as f:
        f.write("\n".join(rows) + "\n")
    data.tofile(basename + ".dat")
    return basename + ".inf"
