"""Dispatch order of the pass-0 cone launches (plan.cpp order_launch_units),
read through the host C ABI (rt_schedule_items): rung by rung, a rung's
transforms interleaved by leaf offset, so that the units reading a stretch of
the rung's series are neighbours, then runs of 21 neighbours dealt to one XCD
each (blocks of 8 * 21 units transposed).  CPU only."""
import math
from collections import Counter, defaultdict

import numpy as np
import pytest

# several rungs, 21 transforms per rung, many pass-0 units per transform
PLAN = dict(size=1 << 18, tsamp=256e-6, period_min=0.1, period_max=1.0, bins_min=240, bins_max=260)


def _items(**kw):
    from riptide_amd import engine
    return engine.schedule_items(**dict(PLAN, **kw))


def _cost(it):
    """plan.cpp item_cost: floats through LDS per merge level, plus load / store."""
    rows = (int(it["s1"]) - int(it["s0"]) + (2 << int(it["levels"]))) if it["tile"] else int(it["node_size"])
    return float(rows) * float(it["bins"]) * (float(it["levels"]) + 2.0)


def _cost_sorted(launch_items):
    """The launch's units longest first: a stable sort by decreasing cost of
    the units in (transform, node, tile) order, the order the planner
    assembles a launch in."""
    base = sorted(launch_items, key=lambda it: (int(it["xform"]), int(it["node_start"]), int(it["s0"])))
    return sorted(base, key=lambda it: -_cost(it))


def _launches(items):
    out = defaultdict(list)
    for it in items:
        out[int(it["launch"])].append(it)
    return [out[k] for k in sorted(out)]


def _key(it):
    return int(it["xform"]), int(it["node_start"]), int(it["node_size"]), int(it["s0"]), int(it["s1"])


@pytest.fixture(scope="module")
def items():
    return _items()


def test_plan_shape(items):
    """The plan exercises the order: several rungs, 21 transforms per rung in
    the 4- and 5-slot pass-0 launches together, many units per transform."""
    p0 = items[items["pass"] == 0]
    assert np.all(p0["src_leaves"] == 1) and np.all(items[items["pass"] > 0]["src_leaves"] == 0)
    rungs = np.unique(p0["rung"])
    assert rungs.size >= 4
    for r in rungs[:-1]:          # the last rung stops at period_max
        assert np.unique(p0[p0["rung"] == r]["bins"]).size == 21
    per_xform = Counter(int(x) for x in p0["xform"])
    assert max(per_xform.values()) >= 8


def test_nothing_lost_or_duplicated(items):
    """(a) every launch holds the units of its cost-sorted order, each once."""
    for launch in _launches(items):
        assert Counter(_key(it) for it in launch) == Counter(_key(it) for it in _cost_sorted(launch))
        assert len({_key(it) for it in launch}) == len(launch)


def test_tile_launches_keep_the_cost_order(items):
    for launch in _launches(items):
        if int(launch[0]["pass"]) == 0:
            continue
        assert [_key(it) for it in launch] == [_key(it) for it in _cost_sorted(launch)]


def test_span_readers_are_neighbours(items):
    """(b) for every pass-0 unit, every unit of its rung whose leaf span
    overlaps its own lies within W = T * ceil(2 Lmax / Lmin) + 2 (8 * 21 - 1)
    positions of it (T the rung's transforms in the launch, Lmin / Lmax its
    shortest / longest unit span in floats; the second term: the XCD
    transposition moves each unit by less than a block of 8 * 21): the bound
    order_launch_units states, under one generation of 512 workgroups."""
    checked = 0
    for launch in _launches(items):
        if int(launch[0]["pass"]) != 0:
            continue
        pos = defaultdict(list)
        for i, it in enumerate(launch):
            a = int(it["node_start"]) * int(it["bins"])
            pos[int(it["rung"])].append((i, a, a + int(it["node_size"]) * int(it["bins"])))
        for r, units in pos.items():
            T = len({int(launch[i]["xform"]) for i, _, _ in units})
            lens = [b - a for _, a, b in units]
            W = T * math.ceil(2 * max(lens) / min(lens)) + 2 * (8 * 21 - 1)
            assert W < 512         # unit spans within 2.5x of each other: all readers within one generation
            idx = np.array([i for i, _, _ in units])
            a = np.array([x for _, x, _ in units])
            b = np.array([x for _, _, x in units])
            for k in range(len(units)):
                over = (a < b[k]) & (b > a[k])
                assert np.abs(idx[over] - idx[k]).max() <= W, (r, k, W)
                checked += 1
    assert checked > 1000


def test_one_transform_per_rung_keeps_the_cost_order():
    """(c) bins_min == bins_max: one transform per rung, so every launch is in
    the cost order alone."""
    for bins in (240, 258):
        its = _items(bins_min=bins, bins_max=bins)
        assert its.size > 100
        for launch in _launches(its):
            assert [_key(it) for it in launch] == [_key(it) for it in _cost_sorted(launch)]


def test_rungs_by_decreasing_cost(items):
    """The rungs of a pass-0 launch in order of their longest unit, so the
    launch tail is made of the cheapest rung's units."""
    for launch in _launches(items):
        if int(launch[0]["pass"]) != 0:
            continue
        worst = {}
        for it in launch:
            r = int(it["rung"])
            worst[r] = max(worst.get(r, 0.0), _cost(it))
        assert worst[int(launch[0]["rung"])] == max(worst.values())
        assert worst[int(launch[-1]["rung"])] == min(worst.values())
