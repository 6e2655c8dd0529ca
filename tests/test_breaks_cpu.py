"""Breakable units without a GPU (include/phyx_amd.h BREAKS): the ABI, and the specification (tests/break_spec.py) on one body per kind
under gravity, at the strict comparison, and at the settling of a step's events."""
import ctypes as C

import numpy as np
import pytest

from phyx_amd import api
import angle_spec
import break_spec
import link_spec
import pin_spec
import slider_spec

F = np.float32
DT = 1.0 / 60.0
G = -200.0
O, Y = (0.0, 0.0), (0.0, 1.0)
KINDS = ("pin", "link", "angle", "slider")


# ---- the ABI ----
def test_break_event_is_32_bytes():
    d = api.break_event_dtype
    assert d.itemsize == 32
    assert [d.fields[f][1] for f in ("kind", "index", "body1", "body2", "step", "reaction", "threshold", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert api.UNIT_KINDS == KINDS == break_spec.KINDS


def test_the_library_has_the_calls(built_lib):
    lib = C.CDLL(built_lib) if isinstance(built_lib, str) else built_lib
    for name in ("phx_world_set_break_limits", "phx_world_get_break_limits", "phx_world_break_events"):
        assert hasattr(lib, name), name


# ---- one body per kind ----
def _pins(rows):
    p = np.zeros(len(rows), dtype=api.pin_dtype)
    for k, (a, b, a1, a2) in enumerate(rows):
        p[k] = (a, b, a1, a2, (0.0, 0.0))
    return p


def _one_body(kind):
    """a body at (0, 100) under gravity, held by: a world pin at its centre; a world rod of 10 from above; an angle lock against the
    torque of a world pin 3 off its centre; a world slider locked on a vertical rail -> (bodies, [pins, links, angles, sliders], the
    kind whose unit 0 carries the load)"""
    bodies = pin_spec.make_bodies([(0.0, 100.0, 3.0, 1.0, False)])
    lists = [_pins([]), link_spec.make_links([]), angle_spec.make_angles([]), slider_spec.make_sliders([])]
    if kind == "pin":
        lists[0] = _pins([(0, -1, O, (0.0, 100.0))])
    elif kind == "link":
        lists[1] = link_spec.make_links([(0, -1, O, (0.0, 110.0), 10.0, 10.0)])
    elif kind == "angle":
        lists[0] = _pins([(0, -1, (-3.0, 0.0), (-3.0, 100.0))])
        lists[2] = angle_spec.make_angles([(0, -1, 0.0, 0.0)])
    else:
        lists[3] = slider_spec.make_sliders([(0, -1, O, (0.0, 100.0), Y, 0.0, 0.0)])
    return bodies, lists, KINDS.index(kind)


def _run(kind, limit, steps, dt=DT):
    """-> (per step the events, per step R of the loaded unit before the step's removals, the lists at the end)"""
    bodies, lists, k = _one_body(kind)
    limits = break_spec.no_limits(lists)
    if limit is not None:
        limits[k][0] = limit
    events, loads = [], []
    for s in range(steps):
        before = [l.copy() for l in lists]
        ev, after, kept = break_spec.step_free(bodies, before, limits, None, dt, G, step=s)
        loads.append(break_spec.reactions(before)[k][0] if len(before[k]) else None)
        events.append(ev)
        lists, limits = after, kept
    return events, loads, lists


@pytest.mark.parametrize("kind", KINDS)
def test_one_body_breaks_at_half_its_load_and_holds_at_twice(kind):
    k = KINDS.index(kind)
    _, loads, _ = _run(kind, None, 60)
    r = loads[-1]
    assert r > 0 and np.isfinite(r), "the limitless run's unit carries nothing: the test would be vacuous"
    load = F(r) / F(DT)                                          # the static load, a force (a torque) as the limit is
    events, _, lists = _run(kind, F(0.5) * load, 2)
    assert len(events[0]) == 1 and len(lists[k]) == 0, "half the static load must break in step 0"
    e = events[0][0]
    assert (e["kind"], e["index"], e["body1"], e["body2"], e["step"], e["reserved"]) == (k, 0, 0, -1, 0, 0)
    assert e["reaction"] > e["threshold"] == F(F(0.5) * load) * F(DT)
    assert len(events[1]) == 0, "a broken unit is gone: it cannot break again"
    events, loads, lists = _run(kind, F(2.0) * load, 60)
    assert all(len(ev) == 0 for ev in events) and len(lists[k]) == 1, "twice the static load must hold for 60 steps"
    assert loads[-1] > 0, "the unit that held still carries the body"


# ---- the strict comparison ----
@pytest.mark.parametrize("kind", KINDS)
def test_the_comparison_is_strict(kind):
    dt = 1.0 / 64.0                                              # a power of two: L dt is exact
    k = KINDS.index(kind)
    _, loads, _ = _run(kind, None, 1, dt)
    r = F(loads[0])
    assert r > 0
    limit = F(r / F(dt))
    assert F(limit * F(dt)) == r
    events, _, lists = _run(kind, limit, 1, dt)
    assert len(events[0]) == 0 and len(lists[k]) == 1, "R == L dt does not break"
    below = np.nextafter(limit, F(0))
    events, _, lists = _run(kind, below, 1, dt)
    assert len(events[0]) == 1 and len(lists[k]) == 0, "the next limit below breaks"
    assert events[0][0]["reaction"] == r and events[0][0]["threshold"] == F(below * F(dt)) < r


def test_a_nan_never_breaks_and_an_idle_unit_has_no_reaction():
    pins = _pins([(0, -1, O, O), (1, -1, O, O)])
    pins["impulse"][0] = (np.nan, 1.0)
    lists = [pins, link_spec.make_links([]), angle_spec.make_angles([]), slider_spec.make_sliders([])]
    limits = break_spec.no_limits(lists)
    limits[0][:] = 1.0
    assert len(break_spec.breaks(lists, limits, DT)) == 0
    assert break_spec.reactions(lists)[0][1] == 0


# ---- settle ----
def test_settle_is_remove():
    pins = _pins([(i, -1, O, (10.0 * i, 0.0)) for i in range(5)])
    pins["impulse"][:, 0] = np.arange(5) + 1.0
    links = link_spec.make_links([(i, i + 1, O, O, 10.0, 10.0) for i in range(5)])
    links["impulse"] = -(np.arange(5) + 1.0)
    lists = [pins, links, angle_spec.make_angles([]), slider_spec.make_sliders([])]
    limits = break_spec.no_limits(lists)
    limits[0][:] = [0.5, 100.0, 0.5, 200.0, 0.5]                 # the first, the middle and the last pin break at dt = 1
    limits[1][:] = [10.0, 20.0, 2.5, 40.0, 50.0]                 # and link 2
    events = break_spec.breaks(lists, limits, 1.0, step=7)
    assert [(e["kind"], e["index"]) for e in events] == [(0, 0), (0, 2), (0, 4), (1, 2)], "(kind, index) ascending"
    assert set(events["step"]) == {7} and list(events["body1"]) == [0, 2, 4, 2] and list(events["body2"]) == [-1, -1, -1, 3]
    assert list(events["reaction"]) == [1.0, 3.0, 5.0, 3.0]
    after, kept = break_spec.settle(lists, limits, events)
    assert after[0].tobytes() == np.delete(pins, [0, 2, 4]).tobytes() and after[1].tobytes() == np.delete(links, [2]).tobytes()
    assert list(kept[0]) == [100.0, 200.0] and list(kept[1]) == [10.0, 20.0, 40.0, 50.0], "the limits follow their units"
    assert len(after[2]) == len(after[3]) == len(kept[2]) == len(kept[3]) == 0
