"""CPU-only tests: the C-ABI library loads and exports every symbol of
include/riptide_amd.h; the host planner (ladder, trial grid, pass schedule) is
bit-exact with the reference; host-side Python logic (width trials, ffafreq,
clustering, peak detection, argument validation) matches the reference.
No compute call reaches the GPU here."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import inputs
from conftest import REPO

HEADER = os.path.join(REPO, "include", "riptide_amd.h")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def lib():
    from riptide_amd import _lib
    return _lib.load()


def test_header_symbols_exported(lib):
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(rt_\w+)\s*\(", text, re.M))
    assert len(declared) >= 25
    from riptide_amd import _lib
    for name in declared:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, f"{name} has no ctypes signature"
    # and nothing in the loader that the header does not declare
    assert set(_lib.EXPORTED) <= declared


def test_test_hooks_only_in_test_build(lib):
    """The fault-injection entry point is not part of the product library;
    the test build (libriptide_amd_testhooks.so) carries it."""
    import ctypes as ct
    from riptide_amd import _lib
    assert not hasattr(lib, "rt_test_corrupt_next_plans")
    assert "rt_test_corrupt_next_plans" not in _lib.EXPORTED
    t = ct.CDLL(_lib.TESTHOOKS_PATH, mode=ct.RTLD_LOCAL)
    assert hasattr(t, "rt_test_corrupt_next_plans")
    text = open(os.path.join(os.path.dirname(HEADER), "riptide_amd_test.h")).read()
    assert "int rt_test_corrupt_next_plans(int on);" in text


def _ladder(lib, n, c):
    fused = ctypes.c_int(-1)
    rungs = ctypes.c_uint64()
    rc = lib.rt_ladder_check(n, c["tsamp"], c["pmin"], c["pmax"], c["bmin"], c["bmax"], ctypes.byref(fused),
                             ctypes.byref(rungs))
    assert rc == 0, lib.rt_last_error()
    return fused.value, rungs.value


def test_ladder_path_choice(lib):
    """The fused ladder indexes samples in 32 bits: series of 2^29 samples or
    more take the per-rung (64-bit) kernel (the planner enforces
    the fused kernel's index range instead of assuming it)."""
    c = dict(tsamp=256e-6, pmin=0.1, pmax=10.0, bmin=240, bmax=260)
    assert _ladder(lib, 1 << 23, c)[0] == 1            # cfg2: fused
    assert _ladder(lib, (1 << 29) - 1, c)[0] == 1
    assert _ladder(lib, 1 << 29, c)[0] == 0            # 2^29: per-rung
    assert _ladder(lib, (1 << 30) + 7, c)[0] == 0
    f, r = _ladder(lib, 1 << 23, c)
    assert r > 0
    # with the 512-float margin every BASELINE config and cfg5's
    # short / medium ranges still take the fused ladder (cfg4's largest factor
    # is ~310); cfg5's long range (factors up to ~1950) takes the fused ladder
    # for its rungs inside the margin and the per-rung kernel for the rest (2)
    cfg4 = dict(tsamp=64e-6, pmin=0.002, pmax=0.5, bmin=16, bmax=32)
    assert _ladder(lib, 1 << 22, cfg4)[0] == 1
    assert _ladder(lib, 2343750, dict(tsamp=256e-6, pmin=0.5, pmax=2.0, bmin=240, bmax=260))[0] == 1   # cfg1
    assert _ladder(lib, 1 << 22, dict(tsamp=256e-6, pmin=0.2, pmax=5.0, bmin=240, bmax=260))[0] == 1   # cfg3
    for rng in inputs.CFG5["ranges"]:
        s = rng["ffa_search"]
        want = 2 if rng["name"] == "long" else 1
        assert _ladder(lib, inputs.CFG5["n"], dict(tsamp=inputs.CFG5["tsamp"], pmin=s["period_min"],
                                                   pmax=s["period_max"], bmin=s["bins_min"],
                                                   bmax=s["bins_max"]))[0] == want, rng["name"]
    # the margin's edge: largest factor with ceil(f) + 2 == 512 is fused,
    # one more sample of window is not (that rung alone to the per-rung kernel)
    assert _ladder(lib, 1 << 20, inputs.LADDER_EDGE_CASE)[0] == 1
    over = dict(inputs.LADDER_EDGE_CASE, pmin=inputs.LADDER_EDGE_CASE["pmin"] * 510.5 / 509.5125)
    over["pmax"] = over["pmin"] * 1.125 ** 2 * 0.999
    # ladder_split: the f = 453.8 rung stays fusable, so the fused list is not
    # empty and the plan is hybrid (2), never all per-rung (0): one rung fused,
    # the f = 510.5 one (ceil(f) + 2 == 513) in the per-rung kernel
    assert _ladder(lib, 1 << 20, over)[0] == 2
    lay = _layout(1 << 20, over)
    assert lay["mode"] == 2 and lay["margin"] == 512
    assert [int(f) for f in lay["rungs"]["f"]] == [453, 510] and lay["rungs"]["fused"].tolist() == [1, 0]
    # every rung past the margin: nothing for the fused kernel
    assert _ladder(lib, 1 << 22, dict(tsamp=64e-6, pmin=40.0, pmax=100.0, bmin=960, bmax=1040))[0] == 0


def _layout(n, c):
    from riptide_amd import engine
    return engine.ladder_layout(n, c["tsamp"], c["pmin"], c["pmax"], c["bmin"], c["bmax"])


def test_ladder_layout_matches_the_planner(lib):
    """rt_ladder_layout agrees with rt_ladder_check and with the ladder of
    periodogram.hpp:135-168 restated here: factors f_r = pmin / (tsamp bmin)
    ((bmax + 1) / bmin)^r, lengths floor(n / f), slots in ladder order that do
    not overlap, each starting on a multiple of four floats."""
    cases = [(c["n"], c) for c in inputs.PGRAM_CASES + inputs.LADDER_ORACLE_CASES]
    cases.append((inputs.CFG5["n"], dict(tsamp=inputs.CFG5["tsamp"], pmin=2.0, pmax=120.0, bmin=960, bmax=1040)))
    for n, c in cases:
        lay = _layout(n, c)
        rungs = lay["rungs"]
        assert (lay["mode"], rungs.size) == _ladder(lib, n, c)
        assert rungs.size > 0 and np.all(rungs["reserved"] == 0)
        ini, geo = c["pmin"] / (c["tsamp"] * c["bmin"]), (c["bmax"] + 1.0) / c["bmin"]
        ladder = ini * geo ** np.arange(400.0)
        for r in rungs:
            assert np.any(np.abs(ladder - r["f"]) <= 4e-16 * r["f"]), r["f"]
            assert r["n"] == int(np.floor(n / r["f"])) >= c["bmin"]
        assert np.all(np.diff(rungs["f"]) > 0)
        assert rungs["leaf_off"][0] == 0 and np.all(rungs["leaf_off"] % 4 == 0)
        ends = (rungs["leaf_off"] + rungs["n"] + 3) // 4 * 4
        # (a rung whose transforms all lie past period_max keeps its slot and is not listed)
        assert np.all(ends[:-1] <= rungs["leaf_off"][1:]) and ends[-1] <= lay["leaf_floats"]
        if c in inputs.LADDER_ORACLE_CASES:
            assert np.array_equal(ends[:-1], rungs["leaf_off"][1:]) and ends[-1] == lay["leaf_floats"]
        fused = rungs["fused"].astype(bool)
        if lay["mode"] == 0:
            assert not fused.any() and lay["margin"] == 0
        else:
            wide = np.ceil(rungs["f"]) + 2 > 512
            assert np.array_equal(fused, ~wide) and (lay["mode"] == 2) == bool(wide.any())
            fmax = rungs["f"][fused & (rungs["f"] != 1.0)].max(initial=0.0)
            assert lay["margin"] == min(512, (int(max(2.0, np.ceil(fmax) + 2)) + 63) // 64 * 64)
    # a truncated list: the count is the whole ladder's, only `cap` records are written
    c = inputs.LADDER_ORACLE_CASES[0]
    two = np.zeros(3, dtype=_layout(c["n"], c)["rungs"].dtype)
    count = ctypes.c_uint64()
    from riptide_amd._lib import ptr
    assert lib.rt_ladder_layout(c["n"], c["tsamp"], c["pmin"], c["pmax"], c["bmin"], c["bmax"], ptr(two), 2,
                                ctypes.byref(count), None, None, None) == 0
    assert count.value == 22 and two["f"][1] == 1.125 and two["n"][2] == 0
    assert lib.rt_ladder_layout(c["n"], c["tsamp"], 0.0, c["pmax"], c["bmin"], c["bmax"], None, 0, None, None, None,
                                None) == 1


def test_ladder_oracle_cases_cover_the_kernel():
    """inputs.LADDER_ORACLE_CASES (tests/test_gpu_ladder.py) really holds the
    classes the ladder kernels branch on, by the plans' own layout: a
    condition on the case list -- if a class goes missing, the list is what
    to fix."""
    src = open(os.path.join(REPO, "riptide_amd", "csrc", "ladder_kernels.hip")).read()
    assert int(re.search(r"^constexpr uint32_t kDsPairSpan = (\d+);$", src, re.M).group(1)) == inputs.LADDER_SPAN
    names = [c["name"] for c in inputs.LADDER_ORACLE_CASES]
    assert len(set(names)) == len(names)
    lays = {c["name"]: _layout(c["n"], c) for c in inputs.LADDER_ORACLE_CASES}
    small, large, integral, identity, blocks, clipped = set(), set(), [], 0, {}, 0
    for c in inputs.LADDER_ORACLE_CASES:
        lay = lays[c["name"]]
        assert 4000 <= c["n"] <= 140000
        assert lay["mode"] in (1, 2)
        blocks[c["name"]] = -(-c["n"] // (inputs.LADDER_SPAN - lay["margin"]))
        for r in lay["rungs"][lay["rungs"]["fused"] == 1]:
            f = float(r["f"])
            if f == 1.0:
                identity += 1
            elif f < 12:
                small.add(int(f))
            else:
                large.add(int(f))
            if f > 1.0 and f == int(f):
                integral.append(int(f))
            # the last window's end, computed as the kernels do, reaches n: min(floor(end), n - 1) clips it
            clipped += f > 1.0 and float(r["n"] - 1) * f + f >= c["n"]
    # (a) every template instance of the fused kernel, and the identity rung
    assert small == set(range(1, 12)) and identity >= 1
    # (b) floor(f) >= 12 at every residue mod 8: output_large's 8-wide loop
    # leaves (F - 2) mod 8 samples, which take the 2-wide loop zero to three
    # times and the odd single read or not; one and several turns of the 8-wide loop
    assert {F % 8 for F in large} == set(range(8))
    assert any(F < 18 for F in large) and any(F >= 26 for F in large)
    # (c) exactly integral factors, powers of two up to 256, below and above
    # the F = 12 switch; and their neighbours one part in 2^40 below
    assert set(integral) >= {2, 4, 8, 16, 32, 64, 128, 256}
    below = lays["pow2_below"]["rungs"]["f"]
    assert [int(f) for f in below] == [1, 3, 7, 15, 31, 63, 127, 255]
    assert np.all(np.ceil(below) - below < 1e-9) and np.all(np.ceil(below) - below > 0)
    # (d) both fused modes, the widest margin, a hybrid whose per-rung part
    # has several rungs, blocks beyond each rung's first and unstaged windows
    assert {lay["mode"] for lay in lays.values()} == {1, 2}
    edge = lays["margin512"]
    assert edge["mode"] == 1 and edge["margin"] == 512 and np.ceil(edge["rungs"]["f"].max()) + 2 == 512
    hyb = lays["hybrid"]
    wide = hyb["rungs"][hyb["rungs"]["fused"] == 0]
    assert hyb["mode"] == 2 and wide.size >= 2 and (hyb["rungs"]["fused"] == 1).sum() >= 1
    assert wide["f"].min() > 124 and wide["n"][0] > 256          # ds_per_block(f) < 32: 256 unstaged outputs per block
    # (e) first, interior and tail blocks everywhere but in the short case, which is one tail block
    assert blocks.pop("short") == 1 and min(blocks.values()) >= 3, blocks
    assert lays["short"]["rungs"].size >= 10 and inputs.LADDER_ORACLE_CASES[-1]["n"] < inputs.LADDER_SPAN
    spans = {c["name"]: inputs.LADDER_SPAN - lays[c["name"]]["margin"] for c in inputs.LADDER_ORACLE_CASES}
    rem = {c["n"] % spans[c["name"]] - (spans[c["name"]] if c["n"] % spans[c["name"]] > 1 else 0)
           for c in inputs.LADDER_ORACLE_CASES}
    assert {-1, 1} <= rem                     # one less and one more than a multiple of the span
    assert any(c["n"] % 2 for c in inputs.LADDER_ORACLE_CASES) and clipped >= 8


def test_dered_cases_cover_the_kernels(lib):
    """dered_common.CASES x LAYOUTS (tests/test_gpu_dered.py) really reaches
    every kernel form of dereddening and normalisation, by the launchers' own
    predicates (rt_deredden_forms): a condition on the case table -- if a
    form goes missing, the table is what to fix."""
    import dered_common as dc
    from riptide_amd import engine as E
    assert len(set(dc.CASE_NAMES)) == len(dc.CASES)
    src = open(os.path.join(REPO, "riptide_amd", "csrc", "dered_host.hpp")).read()
    assert int(re.search(r"^constexpr uint32_t kNpBufSize = (\d+);$", src, re.M).group(1)) == 8192
    assert int(re.search(r"^constexpr uint32_t kNormBlocks = (\d+);$", src, re.M).group(1)) * 256 == 131072
    seen = {}          # (mode, field) -> values
    by_factor = {}     # scrunch factor -> [(n_lo, tail)]
    for c in dc.CASES:
        assert c["n"] <= 1100000 + 16385, c["name"]
        for lay in dc.LAYOUTS:
            for mode, (dered, norm) in {"dered": (1, 0), "both": (1, 1), "norm": (0, 1)}.items():
                f = E.deredden_forms(c["n"], c["ws"], c["mp"], dered, norm, **dc.forms_args(c, lay))
                for k, v in f.items():
                    seen.setdefault((mode, k), set()).add(v)
                if mode == "dered":
                    assert f["scrunch_factor"] == dc.factor(c) and f["n_lo"] == (c["n"] // dc.factor(c))
                    by_factor.setdefault(f["scrunch_factor"], set()).add((f["n_lo"], c["n"] % f["scrunch_factor"]))
                    # the forms' own definitions, restated
                    sf = f["scrunch_factor"]
                    n2 = sf // 2 - sf // 2 % 8
                    staged = sf <= 256 and (sf <= 128 or sf - n2 <= 128)
                    assert (f["scrunch"] == 0) == (sf == 1) and (f["scrunch"] == E.SCRUNCH_GENERAL) == (sf > 1 and not staged)
                    assert f["scrunch_chunks"] == (0 if sf == 1 else -(-sf // 8192))
                    assert f["rmed"] == (E.RMED_SMALL if f["rmed_width"] <= 255 else E.RMED_LARGE)
                    assert (f["subtract"] == E.SUBTRACT_PER_SAMPLE) == (sf == 1)
    # every form of every stage
    assert seen["dered", "scrunch"] == {0, E.SCRUNCH_STAGED_VEC, E.SCRUNCH_STAGED, E.SCRUNCH_GENERAL}
    assert seen["dered", "rmed"] == {E.RMED_SMALL, E.RMED_LARGE}
    assert seen["dered", "subtract"] == {E.SUBTRACT_PER_SAMPLE, E.SUBTRACT_SLOPE1, E.SUBTRACT_SLOPE4}
    assert seen["dered", "fused"] == {0} and seen["both", "fused"] == {0, 1} and seen["norm", "subtract"] == {0}
    for mode in ("both", "norm"):
        assert seen[mode, "norm_partial"] >= {E.NORM_SCALAR, E.NORM_VEC}
        assert seen[mode, "norm_apply"] == {E.NORM_SCALAR, E.NORM_VEC} and seen[mode, "norm_passes"] >= {1, 2}
    # the statistics kernels' loops on each side of one grid: n / 4 and n against 131072
    long = next(c for c in dc.CASES if c["name"] == "long_f5")
    assert long["n"] // 4 > 2 * 131072 and long["n"] % 4 == 3 and (long["n"] // 4) % 131072 not in (0, 131071)
    for lay, part in (("aligned", E.NORM_VEC), ("in_off", E.NORM_SCALAR)):
        f = E.deredden_forms(long["n"], long["ws"], long["mp"], 0, 1, **dc.forms_args(long, lay))
        assert (f["norm_partial"], f["norm_passes"]) == (part, 2)
    assert sum(c["n"] // 4 <= 131072 for c in dc.CASES) > 100
    # the scrunch: every factor of dc.FACTORS, each with n_lo = min_points + 1 and n_lo past a 64-output
    # block, and tails of 0, 1 and factor - 1 samples; staged factors at 129-248, 256 (64 KiB of LDS),
    # the general kernel at 249-255 and above 256, and on each side of numpy's buffer size
    for sf in dc.FACTORS:
        los, tails = {lo for lo, _ in by_factor[sf]}, {t for _, t in by_factor[sf]}
        assert min(los) <= 6 and max(los) >= 67 and tails >= {0, 1, sf - 1}, sf
    general = {sf for sf in by_factor if sf > 1 and not (sf <= 128 or (sf <= 256 and sf - (sf // 2 - sf // 2 % 8) <= 128))}
    assert {249, 255, 257, 773} <= general and {129, 200, 248, 256} & general == set()
    assert seen["dered", "scrunch_chunks"] >= {0, 1, 2, 3} and {8192, 8193} <= set(by_factor)
    # the interpolation's edges: one slope, even and odd factors from 2 up, the first factors of the
    # two-segment path, every n mod 4 below one 4096-sample block, and a four-sample group over xp[0] and xp[last]
    small = [c for c in dc.CASES if c["n"] < 4096]
    assert any(c["n"] // dc.factor(c) == 2 for c in small)
    assert {c["n"] % 4 for c in small if dc.factor(c) in (4, 5)} == {0, 1, 2, 3}
    assert {2, 3, 4, 5} <= set(by_factor)
    last_in_group = {(((c["n"] // dc.factor(c)) - 1) * dc.factor(c) + (dc.factor(c) - 1) // 2) % 4
                     for c in dc.CASES if dc.factor(c) >= 4}
    assert last_in_group == {0, 1, 2, 3}
    # refusals, as the device call's
    rec = np.zeros(1, dtype=E.DERED_FORMS_DTYPE)
    from riptide_amd._lib import ptr
    assert lib.rt_deredden_forms(1000, 100, 3, 1, 1, 0, 0, 1000, 1000, ptr(rec)) == 0
    for bad in ((1000, 100, 4, 1, 1, 0, 0),      # even min_points
                (99, 99, 99, 1, 1, 0, 0),         # width not below size
                (1000, 100, 3, 1, 1, 2, 0), (1000, 100, 3, 1, 1, 0, 16)):   # no float address mod 16
        assert lib.rt_deredden_forms(*bad, 1000, 1000, ptr(rec)) == 1, bad
    assert lib.rt_deredden_forms(1000, 100, 3, 1, 1, 0, 0, 1000, 1000, None) == 1


def test_version(lib):
    assert b"gfx950" in lib.rt_version()


def _grid(lib, c):
    L = ctypes.c_size_t()
    rc = lib.rt_periodogram_length(c["n"], c["tsamp"], c["pmin"], c["pmax"], c["bmin"], c["bmax"], ctypes.byref(L))
    assert rc == 0
    periods = np.empty(L.value, np.float64)
    foldbins = np.empty(L.value, np.uint32)
    from riptide_amd._lib import ptr
    assert lib.rt_periodogram_grid(c["n"], c["tsamp"], c["pmin"], c["pmax"], c["bmin"], c["bmax"],
                                   ptr(periods), ptr(foldbins)) == 0
    return periods, foldbins


@pytest.mark.parametrize("case", inputs.PGRAM_CASES, ids=lambda c: c["name"])
def test_grid_small_bit_exact(lib, golden, case):
    periods, foldbins = _grid(lib, case)
    assert np.array_equal(periods, golden[f"pg_{case['name']}_periods"])
    assert np.array_equal(foldbins, golden[f"pg_{case['name']}_foldbins"])


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4"])
def test_grid_full_bit_exact(lib, golden_full, name):
    g = golden_full["configs"][name]
    periods, foldbins = _grid(lib, g["case"])
    assert periods.size == g["length"]
    assert sha(periods) == g["periods_sha"]
    assert sha(foldbins) == g["foldbins_sha"]


@pytest.mark.parametrize("case", inputs.FULL_CASES + inputs.PGRAM_CASES + inputs.SEARCH_CASES,
                         ids=lambda c: c["name"] + str(c["n"]))
def test_schedule_invariants(lib, case):
    u = [ctypes.c_uint64() for _ in range(4)]
    d = [ctypes.c_double() for _ in range(2)]
    rc = lib.rt_schedule_check(case["n"], case["tsamp"], 10, case["pmin"], case["pmax"], case["bmin"], case["bmax"],
                               ctypes.byref(u[0]), ctypes.byref(u[1]), ctypes.byref(u[2]), ctypes.byref(d[0]),
                               ctypes.byref(d[1]), ctypes.byref(u[3]))
    assert rc == 0, lib.rt_last_error()
    assert u[1].value >= u[0].value > 0
    # actual traffic stays within 1.6x the SURVEY.md §8(d) algorithmic bytes
    assert d[1].value <= 1.6 * d[0].value


def test_schedule_cfg2_shape(lib):
    """cfg2 (headline): every cell of every transform is transformed; the plan
    has the documented size (1153 transforms, 1331.6 M cells)."""
    u = [ctypes.c_uint64() for _ in range(4)]
    d = [ctypes.c_double() for _ in range(2)]
    assert lib.rt_schedule_check(1 << 23, 256e-6, 6, 0.1, 10.0, 240, 260, *(ctypes.byref(x) for x in u[:3]),
                                 ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(u[3])) == 0
    assert u[0].value == 1153
    assert abs(u[3].value / 1e6 - 1331.6) < 0.1


def test_schedule_refuses_blocks_over_2gib(lib):
    """A transform block of >= 2^31 bytes would overflow the cone kernel's
    32-bit buffer range: the planner refuses it with ValueError
    text instead of producing silently wrong output.  f == 1 rung: m * p = N."""
    u = [ctypes.c_uint64() for _ in range(4)]
    d = [ctypes.c_double() for _ in range(2)]
    args = (*(ctypes.byref(x) for x in u[:3]), ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(u[3]))
    n = (1 << 29) + 4096                       # 2^31 + 16 KiB of samples at the first rung
    rc = lib.rt_schedule_check(n, 1e-3, 2, 0.24, 0.3, 240, 260, *args)
    assert rc == 1 and b"2 GiB" in lib.rt_last_error()
    n = (1 << 29) - 4096 * 260                 # every block below 2 GiB
    assert lib.rt_schedule_check(n, 1e-3, 2, 0.24, 0.25, 240, 240, *args) == 0, lib.rt_last_error()


def test_snr_shape_sweep_schedules(lib):
    """Every schedule of the fused S/N row-shape sweep (inputs.SNR_SHAPE_RANGES,
    tests/test_gpu_snr_shapes.py) passes the host planner's validation, at
    both sizes: 2^16 samples, where the low rungs take several passes (more
    work items than transforms: the S/N runs on final tiles), and
    5 bins_max + 3 samples, where every transform is one whole unit; and every
    bins value of the range has a transform."""
    for bmin, bmax in inputs.SNR_SHAPE_RANGES:
        for kind, n in inputs.snr_shape_sizes(bmax).items():
            c = inputs.snr_shape_plan(bmin, bmax, n)
            assert c["pmin"] == bmin * c["tsamp"] and c["pmax"] <= 0.99 * n * c["tsamp"]
            u = [ctypes.c_uint64() for _ in range(4)]
            d = [ctypes.c_double() for _ in range(2)]
            rc = lib.rt_schedule_check(n, c["tsamp"], 10, c["pmin"], c["pmax"], bmin, bmax,
                                       *(ctypes.byref(x) for x in u[:3]), ctypes.byref(d[0]), ctypes.byref(d[1]),
                                       ctypes.byref(u[3]))
            assert rc == 0, (bmin, bmax, kind, lib.rt_last_error())
            transforms, items = u[0].value, u[1].value
            assert transforms >= bmax - bmin + 1
            assert (items > transforms) if kind == "tiles" else (items == transforms), (bmin, bmax, kind)
            _, foldbins = _grid(lib, c)
            assert set(range(bmin, bmax + 1)) <= set(foldbins.tolist()), (bmin, bmax, kind)


# Restatement of the row-shape tables the fused S/N is specialised by:
# merge_slots and snr_group (riptide_amd/csrc/common.hpp), the short rows'
# 4-lane groups and the chunk templates snr_epilogue picks
# (riptide_amd/csrc/cone_snr.hpp: kSnrShortG, snr_rows<5|9|17, G>, the
# one-wave-per-row loop past 64 x 17 bins), and snr_seg_ok's 240-264 bins.
def _merge_slots(p):
    if p <= 32:
        return "pack2"
    s = (p + 63) // 64
    for top in (1, 2, 3, 4, 5, 8, 11, 16, 22, 45):
        if s <= top:
            return top
    return 0


def _snr_group(p):
    if p <= 32:
        return 4
    G = 8
    while G < 64 and (((p + G - 1) // G) | 1) > 17:
        G <<= 1
    return G


def _row_class(p):
    G = _snr_group(p)
    c = (p + G - 1) // G
    if p <= 32 or c < 17:
        c |= 1
    chunk = 5 if c <= 5 else 9 if c <= 9 else 17 if c <= 17 else "loop"
    return _merge_slots(p), G, chunk if G < 16 or chunk == "loop" else 17, 240 <= p <= 264


def test_snr_shape_sweep_covers_breakpoints():
    """The sweep's ranges hold both sides of every breakpoint of the row-shape
    tables: p | p + 1 take different instantiations (by the restatement
    above) and one range contains both, so a later edit of the table that
    drops a class fails here."""
    ranges = inputs.SNR_SHAPE_RANGES
    assert len(ranges) == len(set(ranges)) == 18
    edges = {32: "pack2 -> 1 slot, G 4 -> 8", 40: "<5,8> -> <9,8>", 64: "1 -> 2 slots", 72: "<9,8> -> <17,8>",
             128: "2 -> 3 slots", 136: "G 8 -> 16", 192: "3 -> 4 slots", 239: "window -> segmented",
             264: "segmented ends", 272: "G 16 -> 32", 320: "5 -> 8 slots", 512: "8 -> 11 slots",
             544: "G 32 -> 64", 704: "11 -> 16 slots", 1024: "16 -> 22 slots", 1088: "chunks -> very-wide loop",
             1408: "22 -> 45 slots"}
    for p, what in edges.items():
        assert _row_class(p) != _row_class(p + 1), (p, what)
        assert any(lo <= p and p + 1 <= hi for lo, hi in ranges), (p, what)
    # every breakpoint of the restated tables is in the list but two, which
    # the BASELINE-shaped tests hold: 20 | 21 (snr_rows<5,4> -> <9,4>: cfg4's
    # 16-32 bins, test_periodogram_golden[cfg4] and test_full_config_every_row)
    # and 256 | 257 (4 -> 5 slots: the 240-260 bins of cfg1-3)
    found = {p for p in range(2, 2880) if _row_class(p) != _row_class(p + 1)}
    assert found - {20, 256} == set(edges)
    # the segmented form needs widths <= 9 (snr_seg_ok): the ranges that meet
    # 240-264 bins, and only they, carry such a list
    for lo, hi in ranges:
        lists = inputs.snr_shape_widths(lo, hi, [1, 2, 3])
        assert ("narrow" in lists) == (lo <= 264 and hi >= 240)
        assert "narrow" not in lists or (max(lists["narrow"]) <= 9 and lists["narrow"] != sorted(lists["narrow"]))
    assert sum("narrow" in inputs.snr_shape_widths(lo, hi, [1]) for lo, hi in ranges) == 2
    assert _merge_slots(2880) == 45 and _merge_slots(2881) == 0
    # the short rows: the 8 | 9-bin edge of the short-row merge (pack_stride),
    # the shortest (2) and the widest (2880) rows the engine accepts
    for p in (2, 2880):
        assert any(lo <= p <= hi for lo, hi in ranges), p
    assert any(lo <= 8 and 9 <= hi for lo, hi in ranges)
    # every class of the tables is met by some bins value of the sweep
    swept = {_row_class(p)[:3] for lo, hi in ranges for p in range(lo, hi + 1)}
    swept |= {_row_class(p)[:3] for p in list(range(16, 33)) + list(range(240, 266))}   # BASELINE-shaped tests
    assert {_row_class(p)[:3] for p in range(2, 2881)} == swept


def test_periodogram_length_errors(lib):
    from riptide_amd import _lib
    L = ctypes.c_size_t()
    cases = [(0.0, 1.0, 2.0, 240, 260, "tsamp must be > 0"),
             (1e-3, 0.0, 2.0, 240, 260, "period_min must be > 0"),
             (1e-3, 1.0, 0.5, 240, 260, "period_max must be > period_min"),
             (1e-3, 1.0, 2.0, 1, 260, "bins_min must be > 1"),
             (1e-3, 1.0, 2.0, 240, 200, "bins_max must be >= bins_min"),
             (1e-3, 0.1, 2.0, 240, 260, "Must have: period_min >= tsamp * bins_min")]
    for tsamp, pmin, pmax, bmin, bmax, msg in cases:
        rc = lib.rt_periodogram_length(10000, tsamp, pmin, pmax, bmin, bmax, ctypes.byref(L))
        assert rc == _lib.RT_EINVAL
        assert lib.rt_last_error().decode().startswith(msg)


def test_width_trials():
    from riptide_amd import generate_width_trials
    assert list(generate_width_trials(240, ducy_max=0.05)) == [1, 2, 3, 4, 6, 9]
    assert list(generate_width_trials(240)) == [1, 2, 3, 4, 6, 9, 13, 19, 28, 42]
    assert list(generate_width_trials(16)) == [1, 2, 3]


def test_ffafreq():
    # test_ffa_base_functions.py:78-118
    from riptide_amd import ffafreq, ffaprd
    m, p = 42, 127
    dt = np.pi / 1000.0
    s = np.arange(m, dtype=float)
    true_periods = p ** 2 / (p - s / (m - 1.0)) * dt
    assert np.allclose(ffafreq(m * p, p, dt=dt), 1.0 / true_periods)
    assert np.allclose(ffaprd(m * p, p, dt=dt), true_periods)
    assert ffafreq(p, p, dt=dt)[0] == 1.0 / (p * dt)
    for args in ((0, p), (np.pi, p), (m * p, 1), (m * p, np.pi), (m * p, m * p + 1)):
        with pytest.raises(ValueError):
            ffafreq(*args, dt=dt)
    with pytest.raises(ValueError):
        ffafreq(m * p, p, dt=0)


def test_cluster1d():
    from riptide_amd import cluster1d
    assert cluster1d(np.array([]), 1.0) == []
    x = np.array([5.0, 1.0, 1.5, 9.0, 5.2])
    cl = cluster1d(x, 0.6)
    assert [sorted(c.tolist()) for c in cl] == [[1, 2], [0, 4], [3]]
    assert [c.tolist() for c in cluster1d(np.array([1.0, 1.1, 1.2]), 0.5)] == [[0, 1, 2]]


def test_find_peaks_on_reference_snr(golden):
    """Host peak detection on the REFERENCE's S/N reproduces the reference's
    candidate list exactly (the logic is unchanged; see peak_detection.py)."""
    from riptide_amd import Metadata, Periodogram, find_peaks
    for case in inputs.SEARCH_CASES:
        name = case["name"]
        from riptide_amd._lib import load, ptr
        lib = load()
        L = ctypes.c_size_t()
        lib.rt_periodogram_length(case["n"], case["tsamp"], case["pmin"], case["pmax"], case["bmin"],
                                  case["bmax"], ctypes.byref(L))
        periods = np.empty(L.value)
        foldbins = np.empty(L.value, np.uint32)
        lib.rt_periodogram_grid(case["n"], case["tsamp"], case["pmin"], case["pmax"], case["bmin"], case["bmax"],
                                ptr(periods), ptr(foldbins))
        snrs = golden[f"search_{name}_snrs"]
        from riptide_amd import generate_width_trials
        widths = generate_width_trials(case["bmin"], ducy_max=case["ducy_max"])
        pg = Periodogram(widths, periods, foldbins, snrs, metadata=Metadata({"tobs": case["n"] * case["tsamp"],
                                                                             "dm": 0.0}))
        peaks, _ = find_peaks(pg)
        got = np.array([(p.ip, p.iw, p.snr) for p in peaks], dtype=np.float64).reshape(-1, 3)
        assert np.array_equal(got, golden[f"search_{name}_peaks"])


def test_shim_validation_before_device():
    """Argument errors of the drop-in are raised before any device work."""
    from riptide_amd import libcpp
    with pytest.raises(ValueError, match="contiguous"):
        libcpp.ffa2(np.zeros((8, 8), np.float32)[:, ::2])
    with pytest.raises(ValueError, match="incorrect number of dimensions"):
        libcpp.ffa2(np.zeros(8, np.float32))
    with pytest.raises(ValueError, match="same number of elements"):
        libcpp.fused_rollback_add(np.zeros(3), np.zeros(4), 1)
    with pytest.raises(ValueError, match="Downsampling factor"):
        libcpp.downsample(np.zeros(10, np.float32), 0.5)


def test_periodogram_object():
    from riptide_amd import Metadata, Periodogram
    pg = Periodogram(np.array([1, 2]), np.array([1.0, 2.0]), np.array([240, 240], np.uint32),
                     np.zeros((2, 2), np.float32), metadata=Metadata({"tobs": 10.0}))
    assert np.array_equal(pg.freqs, [1.0, 0.5])
    assert pg.tobs == 10.0
    assert Periodogram.from_dict(pg.to_dict()).metadata == pg.metadata
    assert Metadata({})["dm"] is None


def test_ffa_schedules_validate(lib):
    """The pass schedule rt_ffa2 runs for every golden FFA shape, plus edge
    shapes (one row, short / long rows, node sizes around the LDS capacity),
    passes the host validation the kernel relies on (unit blobs: DMA
    segments tile the fill, row-slot tables cover every row once, row pairs
    share head and tail rows)."""
    from tests.golden import inputs
    shapes = {(m, p) for m, p, _ in inputs.FFA_CASES}
    shapes |= {(1, 1), (1, 260), (2, 1), (3, 17), (64, 32), (65, 33), (384, 16), (385, 16), (1000, 31),
               (72, 250), (73, 250), (5000, 257), (4097, 64), (300, 700), (40, 2880)}
    n = ctypes.c_uint64()
    for m, p in sorted(shapes):
        assert lib.rt_ffa_schedule_check(m, p, ctypes.byref(n)) == 0, (m, p, lib.rt_last_error())
        assert n.value >= 1
    assert lib.rt_ffa_schedule_check(0, 16, None) == 1


# ---------------------------------------------------------------- host sanitizers
def _asan_cases():
    from riptide_amd.ffautils import generate_width_trials
    cases = []
    for c in inputs.FULL_CASES:
        w = len(generate_width_trials(c["bmin"], ducy_max=c["ducy_max"], wtsp=1.5))
        cases.append((c["name"], ["pgram", c["n"], c["tsamp"], c["pmin"], c["pmax"], c["bmin"], c["bmax"], w], {}))
    c2 = inputs.FULL_CASES[1]
    w2 = len(generate_width_trials(c2["bmin"], ducy_max=c2["ducy_max"], wtsp=1.5))
    cases.append(("cfg2-bench-1536M", ["pgram", c2["n"], c2["tsamp"], c2["pmin"], c2["pmax"], c2["bmin"], c2["bmax"], w2],
                  {"RIPTIDE_AMD_SCRATCH_MFLOATS": "1536"}))
    cases.append(("cfg2-cosched-384M", ["pgram", c2["n"], c2["tsamp"], c2["pmin"], c2["pmax"], c2["bmin"], c2["bmax"], w2],
                  {"RIPTIDE_AMD_SCRATCH_MFLOATS": "384", "RIPTIDE_AMD_COSCHED": "1"}))
    c5 = inputs.CFG5
    for r in c5["ranges"]:
        f = r["ffa_search"]
        w = len(generate_width_trials(f["bins_min"], ducy_max=0.2, wtsp=f["wtsp"]))
        cases.append((f"cfg5-{r['name']}", ["pgram", c5["n"], c5["tsamp"], f["period_min"], f["period_max"],
                                            f["bins_min"], f["bins_max"], w], {}))
    for m, p in [(1, 1), (2, 1), (7, 3), (33, 64), (150, 260), (1023, 34), (1025, 34), (5000, 260), (21474, 240),
                 (134217, 16), (3000, 17), (777, 4000), (40, 12000), (9, 70000),
                 (999, 9), (1500, 12), (5000, 20), (4099, 24), (2049, 27), (3001, 31), (65537, 32)]:
        cases.append((f"ffa-{m}x{p}", ["ffa", m, p], {}))
    for m, p, _ in inputs.FFA_CASES:
        cases.append((f"ffa-{m}x{p}", ["ffa", m, p], {}))
    return cases


def test_asan_schedule_check():
    """The host planner and the C ABI's host-only entry points under
    AddressSanitizer + UBSan (`make -C riptide_amd/csrc asan`): the period
    grid, the pass schedule with every unit blob / DMA segment table /
    row-slot table (validate_exec_plan), and the ladder choice, for the five
    BASELINE configurations (cfg2 also at bench.py's one-group budget), and
    the single-transform schedules of every ffa2 shape the GPU parity tests
    run.  Any sanitizer report aborts the checker (exit status != 0)."""
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    exe = os.path.join(REPO, "build", "asan", "sched_check")
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    env0 = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
                UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    # ffa shapes whose rows are too wide for the LDS engine (p > 45 x 64
    # bins) take the global-memory path: rt_ffa_schedule_check rejects them

    def run(case):
        name, argv, extra = case
        env = {k: v for k, v in env0.items() if k not in ("RIPTIDE_AMD_SCRATCH_MFLOATS", "RIPTIDE_AMD_COSCHED")}
        env.update(extra)
        r = subprocess.run([exe] + [str(a) for a in argv], env=env, capture_output=True, text=True, timeout=600)
        return name, argv, r

    cases = _asan_cases()
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 2)) as ex:
        results = list(ex.map(run, cases))
    for name, argv, r in results:
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (name, r.stderr[-3000:])
        if argv[0] == "ffa" and argv[2] > 45 * 64:
            assert r.returncode == 1 and "bad shape" in r.stdout, (name, r.stdout, r.stderr[-2000:])
            continue
        assert r.returncode == 0, (name, r.returncode, r.stdout, r.stderr[-3000:])
        if name == "cfg2-bench-1536M":
            assert int(r.stdout.split("launches=")[1].split()[0]) <= 16, r.stdout


@pytest.mark.parametrize("mode", ["fold", "dered", "harmonic"])
def test_asan_host_check(mode):
    """The host planning the C ABI's device files rely on, under
    AddressSanitizer + UBSan (build/asan/host_check, g++, no HIP), every array
    a heap block of exact size.  fold: the accept and EINVAL cases of
    test_fold_host.py and a table of all three modes with staged and unstaged
    factors, every candidate's rows and result inside the reported workspace
    and output.  dered: the four workspace regions over (size, width,
    min_points, batch), scrunch factor 1 and above, and rt_deredden_forms
    against the launchers' predicates over factors, alignments, strides and
    stage selections.  harmonic: the tile
    resolution against the plain rank-order loop for n in {2, 63, 64, 65, 130}
    and 1, 7, n - 1 rows per tile, with near pairs, a tile past the near cap,
    and out-of-range near pairs (the library's own error)."""
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "riptide_amd", "csrc"), "asan"])
    exe = os.path.join(REPO, "build", "asan", "host_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, mode], env=env, capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith(f"host_check {mode} OK")


def test_bench_pmc_summary_matches_sources(tmp_path, monkeypatch):
    """bench.pmc_traffic takes the newest PMC summary measured on the current
    kernel sources (csrc_sha == source_digest()), not merely the newest file
    name, and reports the traffic as stale when none matches."""
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    (tmp_path / "riptide_amd" / "csrc").mkdir(parents=True)
    (tmp_path / "riptide_amd" / "csrc" / "k.hip").write_text("kernel v1")
    (tmp_path / "profiles").mkdir()
    monkeypatch.setattr(bench, "REPO", str(tmp_path))
    cur = bench.source_digest()

    def put(name, sha, hbm):
        (tmp_path / "profiles" / name).write_text(json.dumps({"csrc_sha": sha, "hbm_bytes_per_trial": hbm}))

    put("r06a_pmc_cone.json", "0123", 1.0)
    put("r06f_pmc_cone.json", cur, 2.0)
    put("r06z_pmc_cone.json", "4567", 3.0)           # newest name, other sources
    s, why = bench.pmc_traffic("cfg2")
    assert why == "ok" and s["hbm_bytes_per_trial"] == 2.0 and s["source"].endswith("r06f_pmc_cone.json")
    put("r06f_pmc_cone_cfg3.json", "0123", 1.0)
    s, why = bench.pmc_traffic("cfg3")
    assert s is None and why.startswith("stale")


def test_bench_dump_snr(tmp_path, monkeypatch):
    """bench.dump_snr (--dump-outputs): a small S/N array is written whole; a
    large one as the same seeded rows in every run (every width of a row,
    float32), with their flat (trial x period) row numbers beside them."""
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    snr = torch.arange(3 * 1001 * 6, dtype=torch.float32).reshape(3, 1001, 6)
    bench.dump_snr(torch, str(tmp_path / "whole"), snr)
    assert sorted(os.listdir(tmp_path / "whole")) == ["snr.npy"]
    assert np.array_equal(np.load(tmp_path / "whole" / "snr.npy"), snr.numpy())
    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 1024)
    monkeypatch.setattr(bench, "DUMP_ROWS", 257)
    for d in ("a", "b"):
        bench.dump_snr(torch, str(tmp_path / d), snr)
    got, rows = np.load(tmp_path / "a" / "snr.npy"), np.load(tmp_path / "a" / "snr_rows.npy")
    assert got.dtype == np.float32 and got.shape == (257, 6) and rows.dtype == np.float64 and rows.shape == (257,)
    assert rows.min() >= 0 and rows.max() < 3 * 1001 and np.all(np.diff(rows) >= 0) and np.unique(rows).size > 200
    assert np.array_equal(got, snr.numpy().reshape(-1, 6)[rows.astype(np.int64)])
    assert np.array_equal(got, np.load(tmp_path / "b" / "snr.npy"))
    assert np.array_equal(rows, np.load(tmp_path / "b" / "snr_rows.npy"))
