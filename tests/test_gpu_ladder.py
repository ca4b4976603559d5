"""The downsampling ladder of a periodogram plan (downsample_fused_kernel and
the multi-rung downsample_ladder_kernel through rt_periodogram_ladder_device)
against the oracle's strict restatement of downsample.hpp:44-82, rung by rung
and bit for bit: every leaf of inputs.LADDER_ORACLE_CASES, found in the
workspace through rt_ladder_layout, equals oracle.downsample of the same
series, and nothing else of the workspace is written.  The oracle is built
without value-changing floating-point flags (oracle/Makefile: -ffp-contract=off
-fno-fast-math), so non-finite samples are compared too.
tests/test_host.py::test_ladder_oracle_cases_cover_the_kernel states which
kernel paths the case list reaches."""
import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu

CASES = inputs.LADDER_ORACLE_CASES
KINDS = ("scaled", "offset", "nonfinite")
BATCHES = (1, 2, 3)
ROWS = max(BATCHES)
SENTINEL = 1e30            # fills the input buffer outside the rows: a read past a row's end shows in the sum


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import riptide_amd
    return riptide_amd


def layout_of(case):
    from riptide_amd import engine
    return engine.ladder_layout(case["n"], case["tsamp"], case["pmin"], case["pmax"], case["bmin"], case["bmax"])


def nonfinite_positions(n, span, rs):
    """A few dozen sample indices: both ends of the series, the samples on
    either side of the fused kernel's block boundaries (the first three and
    the last two multiples of `span`), and two dozen seeded ones."""
    pos = {0, 1, n - 2, n - 1}
    bounds = list(range(span, n, span))
    for m in bounds[:3] + bounds[-2:]:
        pos |= {m - 2, m - 1, m, m + 1}
    pos |= set(rs.choice(n, size=24, replace=False).tolist())
    return np.array(sorted(p for p in pos if 0 <= p < n))


def series(case, kind, span):
    """ROWS deterministic series of the case's length, float32.
    scaled: normal noise times 10^uniform(-3, 3) per sample, so any change of
    the order of additions changes bits.  offset: the same plus 1000.
    nonfinite: scaled with +inf, -inf and NaN at nonfinite_positions (the
    three values in turn, starting one further on in each row)."""
    n = case["n"]
    rs = np.random.RandomState(1000 + CASES.index(case))
    x = rs.normal(size=(ROWS, n)) * 10.0 ** rs.uniform(-3.0, 3.0, size=(ROWS, n))
    if kind == "offset":
        x = x + 1000.0
    x = x.astype(np.float32)
    if kind == "nonfinite":
        pos = nonfinite_positions(n, span, rs)
        assert 24 <= pos.size <= 48 and pos[-1] == n - 1
        bad = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)
        for b in range(ROWS):
            x[b, pos] = bad[(np.arange(pos.size) + b) % 3]
    return x


_reference = {}


def reference(oracle, case, kind):
    """(series [ROWS, n], expected leaf buffers [ROWS, leaf_floats] with zeros
    outside the rungs' slots), computed once per (case, kind) and read-only:
    rung i of row b is oracle.downsample(x[b], f_i), the identity rung x[b]."""
    key = (case["name"], kind)
    if key not in _reference:
        lay = layout_of(case)
        x = series(case, kind, inputs.LADDER_SPAN - lay["margin"])
        want = np.zeros((ROWS, lay["leaf_floats"]), dtype=np.float32)
        for b in range(ROWS):
            for r in lay["rungs"]:
                o, m = int(r["leaf_off"]), int(r["n"])
                d = x[b] if r["f"] == 1.0 else oracle.downsample(x[b], float(r["f"]))
                assert d.size == m
                want[b, o:o + m] = d
        x.setflags(write=False)
        want.setflags(write=False)
        _reference[key] = (x, want)
    return _reference[key]


def differing(got, want):
    """Indices where two float32 arrays differ: NaN against non-NaN, or any
    bit of two non-NaN values (so -0.0 differs from 0.0); two NaNs agree
    whatever their payloads."""
    gn, wn = np.isnan(got), np.isnan(want)
    bits = got.view(np.uint32) != want.view(np.uint32)
    return np.flatnonzero((gn != wn) | (bits & ~(gn & wn)))


@pytest.mark.parametrize("per_rung", [False, True], ids=["default", "per_rung"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_ladder_leaves_equal_the_oracle(rt, oracle, monkeypatch, case, per_rung):
    """Every used rung's leaf, for every trial of batches of 1, 2 and 3 whose
    rows lie n + 1 floats apart (neither 8- nor 16-byte aligned rows), equals
    the oracle's downsample of that row; the floats between the rungs' slots
    and the rest of the workspace stay zero.  per_rung: the plan made with
    RIPTIDE_AMD_PER_RUNG_LADDER=1, every rung through the per-rung kernel's
    first-block table."""
    import torch
    from riptide_amd import engine
    if per_rung:
        monkeypatch.setenv("RIPTIDE_AMD_PER_RUNG_LADDER", "1")
    else:
        monkeypatch.delenv("RIPTIDE_AMD_PER_RUNG_LADDER", raising=False)
    n = case["n"]
    plan = engine.PeriodogramPlan(n, case["tsamp"], [1], case["pmin"], case["pmax"], case["bmin"], case["bmax"])
    lay = plan.ladder_layout()
    rungs, leaf = lay["rungs"], lay["leaf_floats"]
    assert rungs.size > 0 and np.array_equal(rungs, layout_of(case)["rungs"])
    failures = []          # every differing rung is listed before the test fails
    for kind in KINDS:
        x, want = reference(oracle, case, kind)
        for B in BATCHES:
            wide = torch.full((B, n + 1), SENTINEL, dtype=torch.float32, device="cuda")
            rows = wide[:, :n]
            rows.copy_(torch.from_numpy(x[:B].copy()))     # the shared reference stays read-only
            assert rows.stride() == (n + 1, 1)
            ws = torch.zeros(plan.workspace_bytes(B), dtype=torch.uint8, device="cuda")
            plan.ladder(rows, ws)
            torch.cuda.synchronize()
            got = ws.cpu().numpy().view(np.float32)
            assert got.size >= B * leaf
            for b in range(B):
                for r in rungs:
                    o, m = int(r["leaf_off"]), int(r["n"])
                    bad = differing(got[b * leaf + o:b * leaf + o + m], want[b, o:o + m])
                    if bad.size:
                        k = int(bad[0])
                        failures.append(f"{kind} B={B} trial {b} rung f={float(r['f'])!r} n={m}: {bad.size} outputs "
                                        f"differ, first k={k}: got {got[b * leaf + o + k]!r} want {want[b, o + k]!r}")
            # the whole workspace: the B leaf buffers with their padding, then zeros
            whole = np.zeros(got.size, dtype=np.float32)
            whole[:B * leaf] = want[:B].reshape(-1)
            stray = differing(got, whole)
            if stray.size and not failures:
                failures.append(f"{kind} B={B}: written outside the rungs' slots at floats {stray[:8].tolist()}")
            # the input is untouched, sentinels included
            back = wide.cpu().numpy()
            assert np.all(back[:, n] == np.float32(SENTINEL))
            assert differing(back[:, :n].ravel(), x[:B].ravel()).size == 0
    print("\n".join(failures))
    assert not failures, (case["name"], len(failures), failures[:4])
