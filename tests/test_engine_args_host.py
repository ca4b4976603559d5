"""CPU-only tests of the Python device layer's plumbing: the error table of
the engine wrappers for bad arguments refused on the host
(tests/golden/engine_errors.json, recorded by tests/golden/make_engine_errors.py
before the shared argument checks existed), and the order in which the slice
pipeline of riptide_amd.dispatch queues and detects."""
import json
import os

import numpy as np
import pytest

import make_engine_errors
from conftest import GOLDEN


def test_error_table_entry_for_entry():
    with open(os.path.join(GOLDEN, "engine_errors.json")) as f:
        table = json.load(f)
    cases = make_engine_errors.cases()
    assert [name for name, _ in cases] == [row[0] for row in table]
    for (name, thunk), row in zip(cases, table):
        assert [name] + (make_engine_errors.outcome(thunk) or ["-", "no error"]) == row


def test_resolve_device_takes_none_int_and_device(monkeypatch):
    import torch
    from riptide_amd.engine import resolve_device
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
    assert resolve_device(None) == torch.device("cuda", 3)
    assert resolve_device(1) == torch.device("cuda", 1)
    assert resolve_device(np.int64(2)) == torch.device("cuda", 2)
    assert resolve_device(torch.device("cuda", 5)) == torch.device("cuda", 5)
    assert resolve_device(torch.device("cuda", 0)).index == 0


E, D = "enqueue", "detect"
# enqueue 0, enqueue 1, detect 0, enqueue 2, detect 1, ..., detect n - 1
PIPELINE_ORDER = {
    0: [],
    1: [(E, 0), (D, 0)],
    2: [(E, 0), (E, 1), (D, 0), (D, 1)],
    5: [(E, 0), (E, 1), (D, 0), (E, 2), (D, 1), (E, 3), (D, 2), (E, 4), (D, 3), (D, 4)],
}


@pytest.mark.parametrize("n", (0, 1, 2, 5))
def test_pipelined_order(n):
    from riptide_amd.dispatch import _pipelined
    log = []

    def steps():
        for k in range(n):
            log.append(("enqueue", k))
            yield f"tag{k}", k

    def detect(k):
        log.append(("detect", k))
        return f"detected{k}"

    want = PIPELINE_ORDER[n]
    pipe = _pipelined(steps(), detect)
    assert log == []                    # nothing is pulled before the first result is asked for
    got = []
    for k, item in enumerate(pipe):
        # item k + 1 was pulled before detect(k) ran, item k + 2 has not been pulled yet
        assert log == want[:want.index(("detect", k)) + 1]
        got.append(item)
    assert log == want
    assert got == [(f"tag{k}", f"detected{k}") for k in range(n)]


def test_pipelined_takes_a_plain_list():
    from riptide_amd.dispatch import _pipelined
    assert list(_pipelined([("a", 1), ("b", 2)], lambda p: -p)) == [("a", -1), ("b", -2)]


def recording_searcher(batch):
    """An EngineSearcher whose device stages record their calls in .log."""
    from riptide_amd.dispatch import EngineSearcher

    class Recording(EngineSearcher):
        def __init__(self):
            super().__init__({"rmed_width": 4.0, "rmed_minpts": 101}, [], device=0, batch=batch)
            self.log, self.queued = [], 0

        def _normalise(self, raw, tsamp):
            self.log.append(("normalise", [int(v) for v in raw[:, 0]]))
            return raw

        def _enqueue_series(self, x, tsamp, dms):
            self.log.append(("enqueue", [int(v) for v in x[:, 0]], list(dms)))
            first, self.queued = self.queued, self.queued + len(dms)
            return {"first": first, "dms": list(dms), "x": x}

        def _detect(self, pend):
            from riptide_amd.peak_detection import Peak
            self.log.append(("detect", pend["first"]))
            # one peak per row; ip is the row's place in the order of enqueueing
            return [[Peak(1.0, 1.0, 1, 0.1, 0, pend["first"] + j, 9.0, dm)] for j, dm in enumerate(pend["dms"])]

    return Recording()


def test_search_device_accel_order_and_attribution(monkeypatch):
    """D = 3 DMs, A = 2 accelerations, batch = 2: the DM slices [0, 1] and [2],
    the row slices [0, 1], [2, 3] and [4, 5].  The sequence is the one the
    hand-written loop gave before the slice pipeline replaced it."""
    import torch
    from riptide_amd import engine
    D, A = 3, 2
    s = recording_searcher(2)

    def resample(x, factors, src=None, out=None, stream=None):
        s.log.append(("resample", [int(x[i, 0]) for i in src], len(factors)))
        return x[torch.as_tensor(np.asarray(src))]

    monkeypatch.setattr(engine, "resample_device", resample)
    raw = torch.arange(float(D))[:, None].repeat(1, 4)          # row d holds d
    accels = [-1.0, 1.0]
    dms = [0.0, 10.0, 20.0]
    out = s.search_device_accel(raw, 1e-3, [{"dm": dm} for dm in dms], accels)
    assert s.log == [
        ("normalise", [0, 1]),
        ("resample", [0, 0], 2), ("enqueue", [0, 0], [0.0, 0.0]),
        ("resample", [1, 1], 2), ("enqueue", [1, 1], [10.0, 10.0]),
        ("detect", 0),
        ("normalise", [2]),
        ("resample", [2, 2], 2), ("enqueue", [2, 2], [20.0, 20.0]),
        ("detect", 2),
        ("detect", 4),
    ]
    assert len(out) == D
    for d, peaks in enumerate(out):
        assert len(peaks) == A
        for a, p in enumerate(peaks):
            r = p.ip                                            # the row, in (DM, accel) order
            assert (r // A, r % A) == (d, a)
            assert p.dm == dms[d] and p.accel == accels[a] and type(p).__name__ == "AccelPeak"
    assert s.search_device_accel(raw, 1e-3, [{"dm": dm} for dm in dms], []) == [[], [], []]
    assert s.search_device_accel(raw[:0], 1e-3, [], accels) == []


@pytest.mark.parametrize("with_callback", (False, True))
def test_submit_samples_order(monkeypatch, with_callback):
    """Series 0, 1 and 3 share a length and series 2 has another, batch = 2:
    the device batches are [0, 1], [3] and [2].  The first batch is queued by
    submit_samples itself, and `uploaded` fires behind the last upload."""
    import torch
    from riptide_amd import reading
    s = recording_searcher(2)
    samples = [np.full(n, float(i), dtype=np.float32) for i, n in enumerate((4, 4, 6, 4))]

    def upload(raws, device=None, stream=None):
        x = torch.from_numpy(np.stack(raws))
        s.log.append(("upload", [int(v) for v in x[:, 0]]))
        return x

    monkeypatch.setattr(reading, "upload_samples", upload)
    monkeypatch.setattr(s, "_enqueue", lambda x, tsamp, metas: s._enqueue_series(x, tsamp, [m["dm"] for m in metas]))
    uploaded = (lambda: s.log.append(("uploaded",))) if with_callback else None
    metas = [{"dm": 10.0 * i} for i in range(4)]
    collect = s.submit_samples(samples, [1e-3] * 4, metas, uploaded=uploaded)
    assert s.log == [("upload", [0, 1]), ("enqueue", [0, 1], [0.0, 10.0])]
    per = collect()
    want = [
        ("upload", [0, 1]), ("enqueue", [0, 1], [0.0, 10.0]),
        ("upload", [3]), ("enqueue", [3], [30.0]),
        ("detect", 0),
        ("upload", [2]), ("uploaded",), ("enqueue", [2], [20.0]),
        ("detect", 2),
        ("detect", 3),
    ]
    assert s.log == [e for e in want if with_callback or e != ("uploaded",)]
    assert [[p.dm for p in peaks] for peaks in per] == [[0.0], [10.0], [20.0], [30.0]]
    assert [peaks[0].ip for peaks in per] == [0, 1, 3, 2]      # series 3 went ahead of series 2
    assert collect() is per and len(s.log) == len(want) - (not with_callback)

    # one batch: uploaded() fires inside submit_samples; none: it still fires, once
    s.log.clear()
    collect = s.submit_samples(samples[:1], [1e-3], metas[:1], uploaded=uploaded)
    want = [("upload", [0]), ("uploaded",), ("enqueue", [0], [0.0])]
    assert s.log == [e for e in want if with_callback or e != ("uploaded",)]
    assert [p.dm for p in collect()[0]] == [0.0]
    s.log.clear()
    collect = s.submit_samples([], [], [], uploaded=uploaded)
    assert s.log == ([("uploaded",)] if with_callback else [])
    assert collect() == [] and s.log == ([("uploaded",)] if with_callback else [])
