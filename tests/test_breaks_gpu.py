"""Breakable units on the device (include/phyx_amd.h BREAKS) held to their specification, tests/break_spec.py: the device World and the
oracle World in the lockstep of tests/unit_lockstep.py, then break_spec.breaks and break_spec.settle on the spec's own lists: every
byte of the state, of the four lists, of the four limit arrays and of the events compared after every step; then the compaction's
edges, the strict comparison through forks of one snapshot, the life cycle and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import phyx_amd
from phyx_amd.api import break_event_dtype
import angle_spec
import break_spec
import link_spec
import pin_spec
import removal_spec
import slider_spec
import unit_lockstep as ul
from unit_lockstep import DT, G, ERR_INVALID, ERR_CAPACITY, ERR_STATE, O, Y
from unit_scenes import mixed_chain as _mixed_chain

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = break_spec.KINDS


def _limits_of(pw):
    return [pw.break_limits(k) for k in range(4)]


def _set_limits(pw, limits):
    """every finite limit of the spec's arrays, set on the device world"""
    for k, lim in enumerate(limits):
        which = np.flatnonzero(np.isfinite(lim))
        if len(which):
            pw.set_break_limits(k, which, lim[which])


def _break_step(oracle, pw, ow, cfg, lists, limits, s, dt=DT):
    """one step of both worlds (unit_lockstep.step), the spec's break test and settling, and the comparison of everything
    -> (the lists and limits as the next step finds them, the step's events)"""
    ul.step(oracle, pw, ow, cfg, lists, dt=dt)
    events = break_spec.breaks(lists, limits, dt)
    got = pw.break_events()
    assert got.dtype == break_event_dtype and got.tobytes() == events.tobytes(), "events differ at step %d: %s / %s" % (s, got, events)
    lists, limits = break_spec.settle(lists, limits, events)
    ul.check(pw, ow, lists, s)
    for k, (a, b) in enumerate(zip(_limits_of(pw), limits)):
        assert a.tobytes() == b.tobytes(), "%s limits differ at step %d" % (KINDS[k], s)
    return lists, limits, events


def _free_peaks(rows, lists, steps, iterations=8):
    """per kind and unit the largest R over `steps` steps of the spec without limits and without contacts, and R of step 0"""
    bodies = pin_spec.make_bodies([r[:5] for r in rows])
    lists = [l.copy() for l in lists]
    limits = break_spec.no_limits(lists)
    peaks = first = None
    for s in range(steps):
        break_spec.step_free(bodies, lists, limits, None, DT, G, iterations)
        r = break_spec.reactions(lists)
        first = first if s else [x.copy() for x in r]
        peaks = [np.maximum(p, x) for p, x in zip(peaks, r)] if s else [x.copy() for x in r]
    return peaks, first


# ---- the lockstep ----
def test_a_chain_under_a_limit(oracle, built_lib):
    """12 links hung level from the world swing down; every pin's limit lies between the top pin's and the bottom pin's peak R of the
    spec's limitless 40 steps: the top of the chain tears off, the links further down hold"""
    rows, pins = pin_spec.chain(12)
    lists = ul.lists(pins=pins)
    peaks, _ = _free_peaks(rows, lists, 40)
    top, bottom = peaks[0][0], peaks[0][11]
    assert top > bottom > 0
    limit = F(F(0.5) * (F(top) + F(bottom)) / F(DT))
    pw, ow = ul.worlds(ul.scene(rows), lists)
    limits = break_spec.no_limits(lists)
    limits[0][:] = limit
    _set_limits(pw, limits)
    assert _limits_of(pw)[0].tobytes() == limits[0].tobytes() and pw.pin_schedule_builds() == 0
    broken = 0
    for s in range(40):
        lists, limits, events = _break_step(oracle, pw, ow, ul.cfg(), lists, limits, s)
        broken += len(events)
    assert broken > 0, "no link broke"
    assert len(lists[0]) == pw.pin_count() == 12 - broken > 0, "no link held"
    assert pw.pin_schedule_builds() >= 2, "a break rebuilds the schedule"


def test_the_four_kinds_in_one_component(oracle, built_lib):
    """_mixed_chain(20) with a limit on every unit.  The spec's limitless run does not break two kinds in one step by itself at limits
    above the peaks, so three units were chosen, the pin, the angle and the slider with the largest R in step 0, and their limits
    lowered to half that R / dt: they break together in step 0, which checks the (kind, index) order across kinds.  The spring links
    are at rest in step 0 and carry nothing then: every link's limit is a twentieth of its peak R of the limitless 14 steps, so that
    links break as soon as they are loaded.  Every other unit's limit is twice its peak R."""
    rows, lists = _mixed_chain(20)
    peaks, first = _free_peaks(rows, lists, 14)
    limits = [(F(2.0) * p / F(DT)).astype(np.float32) for p in peaks]
    limits[1] = (F(0.05) * peaks[1] / F(DT)).astype(np.float32)
    chosen = []
    for k in (0, 2, 3):
        u = int(np.argmax(first[k]))
        assert first[k][u] > 0, "no %s is loaded in step 0" % KINDS[k]
        limits[k][u] = F(0.5) * first[k][u] / F(DT)
        chosen.append((k, u))
    for lim in limits:
        lim[~(lim > 0)] = np.inf                                 # (a unit that never carried anything: any limit holds)
    pw, ow = ul.worlds(ul.scene(rows), lists)
    _set_limits(pw, limits)
    seen = []
    for s in range(14):
        lists, limits, events = _break_step(oracle, pw, ow, ul.cfg(), lists, limits, s)
        seen.append([(int(e["kind"]), int(e["index"])) for e in events])
    assert [e for e in seen[0] if e in chosen] == chosen and {k for k, _ in seen[0]} >= {0, 2, 3}, "the chosen units break in step 0, in (kind, index) order"
    assert all(step == sorted(step) for step in seen)
    assert any(k == 1 for step in seen for k, _ in step), "no link broke"
    assert sum(len(l) for l in lists) == pw.pin_count() + pw.link_count() + pw.angle_count() + pw.slider_count() > 0


def test_a_break_among_contacts(oracle, built_lib):
    """a shelf held by a world pin and an angle lock carries itself at 1.5 times its own weight; a box of 2.25 times its mass lands on
    it and the pin gives way under the landing, not before"""
    rows = [(0.0, 20.0, 4.0, 1.0, False), (0.0, 26.0, 3.0, 3.0, False)]
    lists = ul.lists(pins=ul.pins([(0, -1, O, (0.0, 20.0))]), angles=angle_spec.make_angles([(0, -1, 0.0, 0.0)]))
    _, first = _free_peaks(rows[:1], lists, 1)
    assert first[0][0] > 0
    limits = break_spec.no_limits(lists)
    limits[0][0] = F(1.5) * first[0][0] / F(DT)
    pw, ow = ul.worlds(ul.scene(rows), lists)
    _set_limits(pw, limits)
    touched_at = broke_at = None
    for s in range(40):
        lists, limits, events = _break_step(oracle, pw, ow, ul.cfg(), lists, limits, s)
        if touched_at is None and len(pw.manifolds) > 0:
            touched_at = s
        if len(events):
            assert broke_at is None and (events[0]["kind"], events[0]["index"], events[0]["body1"], events[0]["body2"]) == (0, 0, 0, -1)
            broke_at = s
    assert touched_at is not None and broke_at is not None and broke_at > touched_at, "the pin broke at %s, the box landed at %s" % (broke_at, touched_at)
    assert pw.pin_count() == 0 and pw.angle_count() == 1, "the lock has no limit and stays"


# ---- the compaction's edges ----
N_MAX = 1025


def _row(i):
    return (10.0 * i, 100.0, 3.0, 1.0, False)


def _own_pins(n):
    return ul.pins([(i, -1, O, (10.0 * i, 100.0)) for i in range(n)])


@functools.lru_cache(maxsize=None)
def _hung(n=N_MAX):
    """n independent bodies, each on its own world pin, after one step of the spec without limits -> (the pins, R of each).  The bodies
    do not interact, so the first k of them are the spec's result for a world of k: computed once for the largest n."""
    pins = _own_pins(n)
    lists = ul.lists(pins=pins)
    break_spec.step_free(pin_spec.make_bodies([_row(i) for i in range(n)]), lists, break_spec.no_limits(lists), None, DT, G)
    r = break_spec.reactions(lists)[0]
    assert (r > 0).all()
    pins.flags.writeable = False
    r.flags.writeable = False
    return pins, r


PATTERNS = {"alternate": lambda i, n: i % 2 == 0, "all": lambda i, n: True, "none": lambda i, n: False, "last": lambda i, n: i == n - 1}


@pytest.mark.parametrize("n,pattern", [(n, "alternate") for n in (1, 63, 64, 65, 256, 257, 1025)] + [(257, p) for p in ("all", "none", "last")])
def test_the_compaction_edges(built_lib, n, pattern):
    """limits of half the weight where the pattern says break, twice the weight elsewhere; one step; the events, the survivors and their
    limits are the spec's, and the schedule was rebuilt exactly where something broke"""
    stepped, r = _hung()
    stepped, r = stepped[:n].copy(), r[:n]
    weight = r / F(DT)
    limits = np.array([(F(0.5) if PATTERNS[pattern](i, n) else F(2.0)) * weight[i] for i in range(n)], dtype=np.float32)
    lists = ul.lists(pins=stepped)
    all_limits = [limits, np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32)]
    events = break_spec.breaks(lists, all_limits, DT)
    assert len(events) == sum(PATTERNS[pattern](i, n) for i in range(n))
    (kept, *_), (kept_limits, *_) = break_spec.settle(lists, all_limits, events)
    pw, _ = ul.worlds(ul.scene([_row(i) for i in range(n)]), ul.lists(pins=_own_pins(n)), with_oracle=False)
    pw.set_break_limits("pin", np.arange(n), limits)
    pw.Update(DT, ul.cfg())
    builds = pw.pin_schedule_builds()
    assert builds == 1
    pw.pin_schedule()                                            # (what the next step does first: settle, then the schedule unless current)
    assert pw.pin_schedule_builds() - builds == (1 if len(events) else 0)
    got = pw.break_events()
    assert got.tobytes() == events.tobytes(), "%s / %s" % (got, events)
    assert pw.pin_count() == len(kept) == n - len(events)
    assert pw.pins().tobytes() == kept.tobytes() and pw.break_limits(0).tobytes() == kept_limits.tobytes()


def test_the_trailing_group_breaks_too(built_lib, monkeypatch):
    """n = 65 as one chain above a cap of 16 pins a group: the trailing HBM group's kernels store the impulses the test reads.  Limits
    alternately half and twice each pin's own R of the spec's limitless step on the device's order (1 where a pin carries nothing yet)."""
    monkeypatch.setenv("PHX_PIN_GROUP_PINS", "16")
    n = 65
    rows, pins = pin_spec.chain(n)
    pw, _ = ul.worlds(ul.scene(rows), ul.lists(pins=pins), with_oracle=False)
    sched = pw.pin_schedule()
    groups = len(sched["group_offsets"]) - 1
    assert sched["lds_groups"] == 0 and groups == 1, "one component that no group of 16 takes: the trailing group alone"
    lists = ul.lists(pins=pins.copy())
    break_spec.step_free(pin_spec.make_bodies(rows), lists, break_spec.no_limits(lists), sched["order"], DT, G, pw.pin_iterations)
    r = break_spec.reactions(lists)[0]
    loaded = r > F(1e-30)                                        # (eight sweeps carry the first step's load a few pins down the chain, no further)
    limits = np.array([(F(0.5) if i % 2 == 0 else F(2.0)) * r[i] / F(DT) if loaded[i] else F(1.0) for i in range(n)], dtype=np.float32)
    all_limits = [limits, np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32)]
    events = break_spec.breaks(lists, all_limits, DT)
    assert events["index"].tolist() == [i for i in range(n) if loaded[i] and i % 2 == 0] and 2 <= len(events) < n
    (kept, *_), (kept_limits, *_) = break_spec.settle(lists, all_limits, events)
    pw.set_break_limits(0, np.arange(n), limits)
    pw.Update(DT, ul.cfg())
    builds = pw.pin_schedule_builds()
    pw.pin_schedule()
    assert pw.pin_schedule_builds() == builds + 1 == 2
    assert pw.break_events().tobytes() == events.tobytes()
    assert pw.pin_count() == n - len(events) and pw.pins().tobytes() == kept.tobytes() and pw.break_limits(0).tobytes() == kept_limits.tobytes()


# ---- the strict comparison, through forks of one snapshot ----
def _one_body(kind):
    """tests/test_breaks_cpu.py's one body per kind -> (rows, lists, the loaded kind)"""
    lists = ul.lists()
    if kind == "pin":
        lists[0] = ul.pins([(0, -1, O, (0.0, 100.0))])
    elif kind == "link":
        lists[1] = link_spec.make_links([(0, -1, O, (0.0, 110.0), 10.0, 10.0)])
    elif kind == "angle":
        lists[0] = ul.pins([(0, -1, (-3.0, 0.0), (-3.0, 100.0))])
        lists[2] = angle_spec.make_angles([(0, -1, 0.0, 0.0)])
    else:
        lists[3] = slider_spec.make_sliders([(0, -1, O, (0.0, 100.0), Y, 0.0, 0.0)])
    return [(0.0, 100.0, 3.0, 1.0, False)], lists, KINDS.index(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_the_comparison_is_strict_on_the_device(built_lib, kind):
    dt = 1.0 / 64.0                                              # a power of two: L dt is exact
    rows, lists, k = _one_body(kind)
    pw, _ = ul.worlds(ul.scene(rows), lists, with_oracle=False)
    snap = pw.save()
    pw.Update(dt, ul.cfg())
    r = break_spec.reactions(ul.lists_of(pw))[k][0]
    limit = F(r / F(dt))
    assert r > 0 and F(limit * F(dt)) == r and len(pw.break_events()) == 0
    for fork_limit, breaks in ((limit, False), (np.nextafter(limit, F(0)), True)):
        fork = phyx_amd.World(0, gravity=G)
        fork.load(snap)
        fork.set_break_limits(kind, [0], [fork_limit])
        fork.Update(dt, ul.cfg())
        events = fork.break_events()
        assert len(events) == (1 if breaks else 0), "limit %r against R %r" % (fork_limit, r)
        assert len(ul.lists_of(fork)[k]) == (0 if breaks else 1)
        if breaks:
            e = events[0]
            assert (e["kind"], e["index"], e["body1"], e["body2"], e["step"], e["reserved"]) == (k, 0, 0, -1, 0, 0)
            assert e["reaction"] == r and e["threshold"] == F(fork_limit * F(dt))


# ---- the life cycle ----
def _hung_world(n, limits=None):
    pw, _ = ul.worlds(ul.scene([_row(i) for i in range(n)]), ul.lists(pins=_own_pins(n)), with_oracle=False)
    if limits is not None:
        pw.set_break_limits(0, np.arange(n), np.asarray(limits, dtype=np.float32))
    return pw


def _weight():
    return F(_hung()[1][0] / F(DT))


def _twin_of(state, lists, limits):
    pb = ul.twin(state, lists)
    _set_limits(pb, limits)
    return pb


def _same(pa, pb, what):
    ul.same(pa, pb, what)
    assert [l.tobytes() for l in _limits_of(pa)] == [l.tobytes() for l in _limits_of(pb)], "the limits differ " + what
    assert pa.break_events().tobytes() == pb.break_events().tobytes(), "the events differ " + what


def _limited_mixed_world(steps):
    """_mixed_chain(12) with a distinct finite limit on every unit, twice its peak R and more, stepped -> (the world, its limits)"""
    rows, lists = _mixed_chain(12, top=(0.0, 300.0))
    peaks, _ = _free_peaks(rows, lists, 12)
    limits = [((F(4.0) + F(0.25) * np.arange(len(p), dtype=np.float32)) * (p + F(1e-6)) / F(DT)).astype(np.float32) for p in peaks]
    pw, _ = ul.worlds(ul.scene(rows), lists, with_oracle=False)
    _set_limits(pw, limits)
    for _ in range(steps):
        pw.Update(DT, ul.cfg())
    assert len(pw.break_events()) == 0
    return pw, limits


def test_limits_follow_their_units_through_remove_pins_and_add(built_lib):
    pa, limits = _limited_mixed_world(4)
    state, lists = pa.state(), ul.lists_of(pa)
    pa.remove_pins([5, 1])
    pa.remove_sliders([0])
    lists[0], limits[0] = np.delete(lists[0], [1, 5]), np.delete(limits[0], [1, 5])
    lists[3], limits[3] = np.delete(lists[3], [0]), np.delete(limits[3], [0])
    assert [l.tobytes() for l in _limits_of(pa)] == [l.tobytes() for l in limits]
    pb = _twin_of(state, lists, limits)
    new = pa.add_pins([(3, -1, O, (35.0, 300.0))])
    assert pb.add_pins([(3, -1, O, (35.0, 300.0))]).tolist() == new.tolist()
    assert np.isinf(pa.break_limits("pin")[new[0]]) and pa.break_limits("pin")[:-1].tobytes() == limits[0].tobytes(), "a new unit is unbreakable"
    for s in range(5):
        pa.Update(DT, ul.cfg()); pb.Update(DT, ul.cfg())
        _same(pa, pb, "at step %d after remove_pins" % s)


def test_limits_follow_their_units_through_remove_bodies(built_lib):
    pa, limits = _limited_mixed_world(4)
    state, lists = pa.state(), ul.lists_of(pa)
    removed = [4, 9]
    new = removal_spec.new_index(len(state[0]), removed)
    kept_lists, kept_limits = [], []
    for units, lim in zip(lists, limits):
        keep = np.array([new[p["body1"]] >= 0 and (p["body2"] < 0 or new[p["body2"]] >= 0) for p in units], dtype=bool)
        kept = units[keep].copy()
        kept["body1"] = new[kept["body1"]]
        kept["body2"] = np.where(kept["body2"] < 0, -1, new[np.maximum(kept["body2"], 0)])
        kept_lists.append(kept); kept_limits.append(lim[keep])
    assert sum(len(l) for l in kept_lists) < sum(len(l) for l in lists)
    assert pa.remove_bodies(removed).tolist() == new.tolist()
    assert [l.tobytes() for l in _limits_of(pa)] == [l.tobytes() for l in kept_limits]
    pb = _twin_of(removal_spec.filter(state, removed)[0], kept_lists, kept_limits)
    for s in range(5):
        pa.Update(DT, ul.cfg()); pb.Update(DT, ul.cfg())
        _same(pa, pb, "at step %d after remove_bodies" % s)


def test_save_load_carry_the_limits_and_load_empties_the_queue(built_lib):
    w = _weight()
    pw = _hung_world(4, [F(2.0) * w, F(0.5) * w, np.inf, F(3.0) * w])
    snap = pw.save()
    saved = pw.break_limits(0)
    pw.Update(DT, ul.cfg())
    assert pw.pin_count() == 3                                   # (settles; the event stays queued)
    fork = phyx_amd.World(0, gravity=G)
    fork.load(snap)
    assert fork.break_limits(0).tobytes() == saved.tobytes() and fork.pin_count() == 4
    fork.Update(DT, ul.cfg())
    assert fork.break_events().tobytes() == pw.break_events().tobytes() and fork.pins().tobytes() == pw.pins().tobytes(), "a fork breaks where the original does"
    # an unsettled break and a queued event are the abandoned timeline's: a load discards both
    pw.load(snap)
    pw.Update(DT, ul.cfg())                                        # pin 1 breaks again: pending, unsettled
    pw.load(snap)
    assert len(pw.break_events()) == 0 and pw.pin_count() == 4 and pw.break_limits(0).tobytes() == saved.tobytes()
    pw.Update(DT, ul.cfg())
    assert pw.pin_count() == 3                                   # settled, the event queued
    pw.load(snap)
    assert len(pw.break_events()) == 0 and pw.pin_count() == 4
    # a snapshot of a world whose lists have no column is what it was
    plain, other = _hung_world(4), _hung_world(4)
    other.set_break_limits(0, [1], [np.inf])
    assert np.isinf(other.break_limits(0)).all()
    plain.remove_pins([0, 1, 2, 3]); other.remove_pins([0, 1, 2, 3])
    assert plain.save().to_bytes() == other.save().to_bytes()


def test_set_state_drops_the_limits_and_the_queue(built_lib):
    w = _weight()
    pw = _hung_world(3, [F(0.5) * w, F(2.0) * w, F(2.0) * w])
    pw.Update(DT, ul.cfg())
    assert pw.pin_count() == 2
    pw.set_state(*pw.state())
    assert pw.pin_count() == 0 and len(pw.break_events()) == 0 and len(pw.break_limits(0)) == 0
    pw.add_pins(_own_pins(3))
    assert np.isinf(pw.break_limits(0)).all()
    pw.Update(DT, ul.cfg())
    assert pw.pin_count() == 3 and len(pw.break_events()) == 0


def test_events_accumulate_and_a_small_cap_keeps_them(built_lib):
    w = _weight()
    pw = _hung_world(4)
    for s in range(3):                                           # the first pin left breaks, step after step, and nobody asks
        pw.set_break_limits(0, [0], [F(0.5) * w])
        pw.Update(DT, ul.cfg())
    total = C.c_int64(-1)
    out = np.zeros(3, dtype=break_event_dtype)
    assert pw.L.phx_world_break_events(pw.h, out.ctypes.data_as(C.c_void_p), 2, C.byref(total)) == ERR_CAPACITY and total.value == 3
    assert pw.L.phx_last_error().decode() == "phx_world_break_events: room for 2 events, the queue holds 3"
    assert pw.L.phx_world_break_events(pw.h, None, 0, C.byref(total)) == ERR_CAPACITY and total.value == 3
    events = pw.break_events()
    assert events["step"].tolist() == [0, 1, 2] and events["index"].tolist() == [0, 0, 0] and events["body1"].tolist() == [0, 1, 2]
    assert (events["kind"] == 0).all() and (events["reaction"] > events["threshold"]).all() and pw.pin_count() == 1
    assert len(pw.break_events()) == 0
    pw.set_break_limits(0, [0], [F(0.5) * w])
    pw.Update(DT, ul.cfg())
    assert pw.break_events()["step"].tolist() == [0], "the ordinal starts again behind a successful call"


def test_a_world_without_a_finite_limit_is_a_world_without_the_calls(built_lib):
    rows, lists = _mixed_chain(12, top=(0.0, 300.0))
    pa, _ = ul.worlds(ul.scene(rows), lists, with_oracle=False)
    pb, _ = ul.worlds(ul.scene(rows), lists, with_oracle=False)
    for k in range(4):
        pa.set_break_limits(k, [0], [np.inf])
    for s in range(6):
        pa.Update(DT, ul.cfg()); pb.Update(DT, ul.cfg())
        assert len(pa.break_events()) == 0 and np.isinf(np.concatenate(_limits_of(pa))).all()
        for name, x, y in zip(ul.NAMES, pa.state(), pb.state()):
            assert x.tobytes() == y.tobytes(), "%s differ at step %d" % (name, s)
        assert [u.tobytes() for u in ul.lists_of(pa)] == [u.tobytes() for u in ul.lists_of(pb)]
    assert pa.pin_schedule_builds() == pb.pin_schedule_builds() == 1


# ---- the refusals ----
def _snapshot_of(pw):
    return (pw.bodies.tobytes(),) + tuple(u.tobytes() for u in ul.lists_of(pw)) + tuple(l.tobytes() for l in _limits_of(pw)) + (pw.pin_schedule_builds(),)


def _raw_set(pw, kind, which, limits, count=None):
    w = None if which is None else np.ascontiguousarray(which, dtype=np.int32)
    v = None if limits is None else np.ascontiguousarray(limits, dtype=np.float32)
    n = count if count is not None else len(w)
    return pw.L.phx_world_set_break_limits(pw.h, kind, None if w is None else w.ctypes.data_as(C.c_void_p), None if v is None else v.ctypes.data_as(C.c_void_p), n)


@pytest.mark.parametrize("staged", ["host", "device"])
def test_rejections_leave_the_world_unchanged(built_lib, staged):
    rows, lists = _mixed_chain(12, top=(0.0, 300.0))
    pw, _ = ul.worlds(ul.scene(rows), lists, with_oracle=False)
    pw.set_break_limits("link", [1], [5.0])
    if staged == "device":
        pw.Update(DT, ul.cfg())
    before = _snapshot_of(pw)
    S = "phx_world_set_break_limits: "
    counts = [len(l) for l in lists]
    for kind in (-1, 4):
        assert _raw_set(pw, kind, [0], [1.0]) == ERR_INVALID and ul.message(pw) == S + "kind %d is none of PHX_UNIT_PIN ... PHX_UNIT_SLIDER [0, 3]" % kind
        out = np.zeros(64, dtype=np.float32)
        assert pw.L.phx_world_get_break_limits(pw.h, kind, out.ctypes.data_as(C.c_void_p), 64) == ERR_INVALID
        assert ul.message(pw) == "phx_world_get_break_limits: kind %d is none of PHX_UNIT_PIN ... PHX_UNIT_SLIDER [0, 3]" % kind
    for k, noun in enumerate(KINDS):
        n = counts[k]
        for which, limits, message in (([n], [1.0], "%s index %d out of range [0, %d)" % (noun, n, n)), ([-1], [1.0], "%s index -1 out of range [0, %d)" % (noun, n)),
                                       ([1, 1], [1.0, 2.0], "%s 1 appears twice in one call" % noun),
                                       ([0, 1], [1.0, 0.0], "%s 1: break limit 0 is not > 0" % noun), ([0], [-2.0], "%s 0: break limit -2 is not > 0" % noun),
                                       ([0, 1], [1.0, np.nan], "%s 1: break limit nan is not > 0" % noun), ([0], [-np.inf], "%s 0: break limit -inf is not > 0" % noun)):
            assert _raw_set(pw, k, which, limits) == ERR_INVALID, (noun, which, limits)
            assert ul.message(pw) == S + message
            assert _snapshot_of(pw) == before
        assert _raw_set(pw, k, None, [1.0], count=1) == ERR_INVALID and ul.message(pw) == S + "null array"
        assert _raw_set(pw, k, [0], None, count=1) == ERR_INVALID and ul.message(pw) == S + "null array"
        assert _raw_set(pw, k, [0], [1.0], count=-1) == ERR_INVALID and ul.message(pw) == S + "negative count -1"
        assert _raw_set(pw, k, None, None, count=0) == 0, "an empty call is a no-op"
        out = np.zeros(max(n - 1, 1), dtype=np.float32)
        assert pw.L.phx_world_get_break_limits(pw.h, k, out.ctypes.data_as(C.c_void_p), n - 1) == ERR_CAPACITY
        assert ul.message(pw) == "phx_world_get_break_limits: room for %d %ss, the world has %d" % (n - 1, noun, n)
        assert _snapshot_of(pw) == before
    with pytest.raises(ValueError):
        pw.set_break_limits("weld", [0], [1.0])
    pw.set_break_limits("slider", [0, 1], [np.inf, 7.0])                # +inf is a limit
    assert pw.break_limits(3)[:2].tolist() == [np.inf, 7.0] and pw.break_limits("link")[1] == 5.0
    assert pw.pin_schedule_builds() == before[-1], "set_break_limits keeps the schedule"
    # inside a step every call is refused
    pw.PreSolve(DT)
    total = C.c_int64(0)
    out = np.zeros(64, dtype=np.float32)
    assert _raw_set(pw, 0, [0], [1.0]) == ERR_STATE and ul.message(pw).startswith(S + "the world is between")
    assert pw.L.phx_world_get_break_limits(pw.h, 0, out.ctypes.data_as(C.c_void_p), 64) == ERR_STATE
    assert pw.L.phx_world_break_events(pw.h, None, 0, C.byref(total)) == ERR_STATE and ul.message(pw).startswith("phx_world_break_events: the world is between")
    pw.FinishStep(DT, ul.cfg())
    assert len(pw.break_events()) == 0
