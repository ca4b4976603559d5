"""Shared by the dereddening tests: the case table that
tests/test_gpu_dered.py runs on the device, the buffer layouts every case
runs in, and the series.  tests/test_host.py::test_dered_cases_cover_the_kernels
states, through rt_deredden_forms, which kernel forms the table reaches.

A case is (n, ws, mp, kind): series length, width_samples and min_points of
TimeSeries.deredden, and the kind of data.  The scrunch factor is
int(ws / mp); min_points is small (1, 3, 5) where the factor is the point, so
the series stay short."""
import zlib

import numpy as np

ROWS = 3                   # every layout holds three different series
SENTINEL = 1e30            # fills the buffers outside the rows
NORM_BOUND = 2e-6          # x max(|ref|, 1)

FACTORS = (2, 3, 4, 5, 7, 8, 16, 128, 129, 200, 248, 249, 255, 256, 257, 512, 773, 1025, 4097, 8192, 8193, 10007,
           16385)
LONG_N = 4 * (2 * 131072 + 5) + 3     # norm_partial4_kernel's paired loop runs, then its single load and the tail

# layout -> (input offset, output offset) in floats past a 16-byte boundary, (input, output) stride - align4(n);
# None: rows n floats apart and the output allocated by the engine
LAYOUTS = {
    "aligned": ((0, 0), (0, 0)),
    "in_off": ((1, 0), (0, 0)),
    "out_off": ((0, 1), (0, 0)),
    "strides": ((0, 0), (8, 4)),
    "packed": ((0, 0), None),
}


def _case(name, n, ws, mp, kind="noise"):
    return dict(name=name, n=int(n), ws=int(ws), mp=int(mp), kind=kind)


def _factor_cases():
    out = []
    for f in FACTORS:
        mp = 3 if f % 2 else 5
        # n_lo: the smallest legal value, and one past a 64-output block of scrunch2_kernel
        for n_lo in (mp + 1, 130 if f <= 1025 else 67):
            for tail in sorted({0, 1, f - 1}):
                out.append(_case(f"f{f}_lo{n_lo}_t{tail}", n_lo * f + tail, f * mp + (tail > 0) * (mp - 1), mp))
    return out


CASES = _factor_cases() + [
    # n_lo = 2: one slope; a four-sample group over xp[0] and xp[last] at once
    _case("nlo2_f4", 8, 4, 1), _case("nlo2_f4_t3", 11, 4, 1), _case("nlo2_f5", 10, 5, 1),
    _case("nlo2_f5_t4", 14, 5, 1), _case("nlo2_f2", 5, 2, 1), _case("nlo2_f300", 600 + 299, 300, 1),
    # n mod 4 = 2 on the two-segment path; scrunch_kernel past one 256-output block
    _case("f4_mod2", 4 * 40 + 2, 12, 3), _case("f5_mod2", 5 * 40 + 2, 15, 3), _case("f257_lo259", 257 * 259 + 5, 771, 3),
    # the median's width: scrunch factor 1 on both sides of 255, and min_points up to 301 above a factor
    _case("w101", 1003, 101, 101), _case("w253", 254, 253, 253), _case("w255", 256, 255, 255),
    _case("w255_n3001", 3001, 255, 255), _case("w257", 258, 257, 257), _case("w257_n3001", 3001, 257, 257),
    _case("w301", 1201, 301, 301), _case("mp101_f4", 4 * 102 + 3, 404, 101), _case("mp255_f2", 2 * 256 + 1, 510, 255),
    _case("mp257_f3", 3 * 258 + 2, 771, 257), _case("mp301_f4", 4 * 302, 1204, 301),
    _case("mp101_f154", 30011, 15625, 101),
    # data
    _case("const_f1", 1003, 101, 101, "const"), _case("const_f5", 5003, 15, 3, "const"),
    _case("const_f773", 773 * 70 + 9, 773 * 3, 3, "const"),
    _case("int8_f1", 5003, 101, 101, "int8"), _case("int8_f4", 5003, 404, 101, "int8"),
    _case("int8_f154", 30011, 15625, 101, "int8"), _case("int8_w257", 3001, 257, 257, "int8"),
    _case("zeros_f1", 5003, 101, 101, "zeros"), _case("zeros_f5", 5003, 15, 3, "zeros"),
    _case("zeros_f200", 200 * 130 + 7, 1000, 5, "zeros"),
    # more than 524288 samples: both loops of the statistics kernels
    _case("long_f5", LONG_N, 15, 3),
]
CASE_NAMES = [c["name"] for c in CASES]


def factor(case):
    return int(max(1, case["ws"] / float(case["mp"])))


def series(case):
    """ROWS different float32 series of the case's length.
    noise: unit normal noise on a level of 5 with a slow sine, each row on its
    own scale, so the order of a sum's additions shows in its bits.  const:
    128.0 (every sum exact).  int8: integers within 128 +- 10, as 8-bit files
    give: heavy ties in both medians.  zeros: +0.0 and -0.0 with one sample
    in ten of noise."""
    n, kind = case["n"], case["kind"]
    rs = np.random.RandomState(zlib.crc32(case["name"].encode()) & 0x7FFFFFFF)
    if kind == "const":
        x = np.full((ROWS, n), 128.0)
    elif kind == "int8":
        x = np.clip(np.rint(rs.normal(size=(ROWS, n)) * 4.0 + 128.0), 118.0, 138.0)
    elif kind == "zeros":
        x = np.where(rs.rand(ROWS, n) < 0.5, 0.0, -0.0) + np.where(rs.rand(ROWS, n) < 0.1, rs.normal(size=(ROWS, n)), 0.0)
    else:
        x = (rs.normal(size=(ROWS, n)) + 5.0 + np.sin(np.arange(n) / 700.0)) * np.array([[1.0], [37.5], [0.01]])
    return np.ascontiguousarray(x, dtype=np.float32)


def geometry(case, layout):
    """(input offset, output offset, input stride, output stride) of a layout
    in floats; output offset and stride None: the engine allocates it."""
    n = case["n"]
    (ioff, ooff), pad = LAYOUTS[layout]
    if pad is None:
        return ioff, None, n, None
    s4 = (n + 3) // 4 * 4
    return ioff, ooff, s4 + pad[0], s4 + pad[1]


def forms_args(case, layout):
    """geometry() as rt_deredden_forms takes it: byte addresses mod 16; an
    output the engine allocates is 16-byte aligned with rows n floats apart."""
    ioff, ooff, istride, ostride = geometry(case, layout)
    return dict(in_align=4 * ioff, out_align=4 * (ooff or 0), in_stride=istride,
                out_stride=case["n"] if ostride is None else ostride)
