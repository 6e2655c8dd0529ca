"""Links on the device (include/phyx_amd.h LINKS) held to their specification, tests/link_spec.py, in the lockstep of
tests/unit_lockstep.py; then the schedule's paths, the life cycle by twins, and the refusals.  (What every kind of unit has alike is in
tests/test_units_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import phyx_amd
from phyx_amd import PhxError
from phyx_amd.api import link_dtype
import link_spec
import removal_spec
import unit_lockstep as ul
from unit_lockstep import DT, G, MODES, ERR_INVALID, ERR_STATE, lists
from unit_scenes import alternating_chain as _alternating_chain, mixed_world
from unit_spec import KINDS, LINK

pytestmark = pytest.mark.gpu


def _step(oracle, pw, ow, cfg, units):
    """-> (the schedule, the links' prestep records)"""
    sched, work = ul.step(oracle, pw, ow, cfg, units)
    return sched, work[LINK]


def _lockstep(oracle, pw, ow, cfg, units, steps):
    """-> (the last schedule, per step the links' states)"""
    states = []
    for s in range(steps):
        sched, work = _step(oracle, pw, ow, cfg, units)
        ul.check(pw, ow, units, s)
        states.append(["active" if w.active else ("idle" if w.idle else "inactive") for w in work])
    return sched, states


# ---- one body on one world link ----
@pytest.mark.parametrize("kind", ["rod", "rope", "spring"])
def test_one_body_on_a_world_link(oracle, built_lib, kind):
    if kind == "rod":
        bodies, link = [(27.0, 100.0, 3.0, 1.0, False)], (0, -1, (-3.0, 0.0), (0.0, 100.0), 24.0, 24.0)
    elif kind == "rope":
        bodies, link = [(0.0, 90.0, 3.0, 1.0, False)], (0, -1, (0.0, 1.0), (0.0, 100.0), 0.0, 25.0)
    else:
        bodies, link = [(4.0, 80.0, 3.0, 1.0, False)], (0, -1, (1.0, 0.5), (0.0, 100.0), 10.0, 10.0, 2.0, 0.3)
    links = link_spec.make_links([link])
    pw, ow = ul.worlds(ul.scene(bodies), lists(links=links))
    assert pw.link_count() == 1 and pw.pin_count() == 0
    assert pw.links().tobytes() == links.tobytes(), "before the first step the links wait on the host"
    sched, states = _lockstep(oracle, pw, ow, ul.cfg(), lists(links=links), 60)
    assert sched["lds_groups"] == 1 and len(sched["class_offsets"]) == 2
    flat = [s[0] for s in states]
    if kind == "rope":
        first = flat.index("active")
        assert first > 10 and set(flat[:first]) == {"idle"}, "the rope was idle, then engaged"
        assert links["impulse"][0] <= 0
    else:
        assert set(flat) == {"active"} and links["impulse"][0] != 0
    assert pw.pin_schedule_builds() == 1


# ---- a mixed world among contacts ----
def _bridge(n):
    """behind `n` bodies: two static posts, a 6-plank deck pinned end to end between them, two rod hangers to world points above, a
    crate on a rope under the middle that lands on a stack of 3 boxes (on a static shelf), a box on a spring.
    -> (body rows, pin rows, link rows)"""
    rows = [(-35.0, 150.0, 5.0, 5.0, True), (35.0, 150.0, 5.0, 5.0, True)]
    posts = (n, n + 1)
    first = n + 2
    rows += [(-25.0 + 10.0 * k, 150.0, 4.0, 1.0, False) for k in range(6)]      # joints at -30, -20 .. 30
    pins = [(first, posts[0], (-5.0, 0.0), (5.0, 0.0))]
    pins += [(first + k, first + k - 1, (-5.0, 0.0), (5.0, 0.0)) for k in range(1, 6)]
    pins += [(first + 5, posts[1], (5.0, 0.0), (-5.0, 0.0))]
    links = [(first + 1, -1, (0.0, 0.0), (-15.0, 180.0), 30.0, 30.0), (first + 4, -1, (0.0, 0.0), (15.0, 180.0), 30.0, 30.0)]
    crate = first + 6
    rows += [(0.0, 140.0, 3.0, 3.0, False)]
    links += [(crate, first + 2, (0.0, 3.0), (5.0, -1.0), 0.0, 18.0)]      # 6 long now: taut after a fall of 12, about 21 steps
    rows += [(0.0, 92.7, 20.0, 2.0, True)] + [(0.0, 99.7 + 10.0 * k, 5.0, 5.0, False) for k in range(3)]      # the shelf and its stack: top at 124.7, 12.3 below the crate
    box = crate + 5
    rows += [(70.0, 150.0, 3.0, 3.0, False)]
    links += [(box, -1, (0.0, 0.0), (60.0, 160.0), 5.0, 5.0, 1.5, 0.5)]
    return rows, pins, links


@pytest.mark.parametrize("mode", list(MODES))
def test_links_among_contacts(oracle, built_lib, mode):
    rows, pin_rows, link_rows = _bridge(0)
    pins, links = ul.pins(pin_rows), link_spec.make_links(link_rows)
    pw, ow = ul.worlds(ul.scene(rows), lists(pins=pins, links=links))
    touched, rope = False, set()
    for s in range(40):
        sched, work = _step(oracle, pw, ow, ul.cfg(MODES[mode]), lists(pins=pins, links=links))
        ul.check(pw, ow, lists(pins=pins, links=links), s)
        rope.add("idle" if work[2].idle else "active")
        m = pw.manifolds
        touched = touched or bool(((m["body1"] == 8) | (m["body2"] == 8)).any())
    assert pw.pin_schedule_builds() == 1
    assert touched, "the crate never landed on the stack"
    assert rope == {"idle", "active"}, "the rope was slack, then taut"
    assert np.abs(links["impulse"][[0, 1, 3]]).min() > 0 and np.abs(pins["impulse"]).max() > 0


# ---- the paths ----
def _alternating_pairs(count):
    bodies, pins, links = [], [], []
    for k in range(count):
        x, y = 40.0 * (k % 20), 30.0 * (k // 20)
        bodies += [(x, y, 4.0, 1.5, False), (x + 10.0, y, 3.0 + (k % 3), 2.0, False)]
        if k % 2:
            links += [(2 * k, 2 * k + 1, (4.0, 1.0 - 0.1 * (k % 7)), (-3.0, 0.0), 2.5, 2.5)]
        else:
            pins += [(2 * k, 2 * k + 1, (5.0, 1.0 - 0.1 * (k % 7)), (-5.0, 0.0))]
    return bodies, pins, links


@pytest.mark.parametrize("case", ["pairs300_cap64", "chain40_cap16", "chain40", "chain300"])
def test_the_paths(oracle, built_lib, monkeypatch, case):
    """several LDS groups; the trailing group out of HBM; one workgroup, two classes; a chain that no workgroup takes"""
    if case == "pairs300_cap64":
        monkeypatch.setenv("PHX_PIN_GROUP_PINS", "64")
        bodies, pin_rows, link_rows = _alternating_pairs(300)
        steps, lds, groups = 4, 5, 5
    elif case == "chain300":
        bodies, pin_rows, link_rows = _alternating_chain(300)
        steps, lds, groups = 3, 0, 1
    else:
        if case == "chain40_cap16":
            monkeypatch.setenv("PHX_PIN_GROUP_PINS", "16")
        bodies, pin_rows, link_rows = _alternating_chain(40)
        steps = 8
        lds, groups = (0, 1) if case == "chain40_cap16" else (1, 1)
    pins, links = ul.pins(pin_rows), link_spec.make_links(link_rows)
    pw, ow = ul.worlds(ul.scene(bodies), lists(pins=pins, links=links))
    sched, _ = _lockstep(oracle, pw, ow, ul.cfg(), lists(pins=pins, links=links), steps)
    assert sched["lds_groups"] == lds and len(sched["group_offsets"]) - 1 == groups
    if case != "pairs300_cap64":
        assert len(sched["class_offsets"]) - 1 == 2, "a chain needs two classes"
    assert np.abs(pins["impulse"]).max() > 0 and np.abs(links["impulse"]).max() > 0


# ---- the life cycle, by twins ----
def _mixed_world():
    return mixed_world("link")


def test_remove_links(built_lib):
    pa = _mixed_world()
    for _ in range(5):
        pa.Update(DT, ul.cfg())
    state, pins, links = pa.state(), pa.pins(), pa.links()
    builds = pa.pin_schedule_builds()
    assert np.abs(links["impulse"]).max() > 0
    pa.remove_links([5, 1])
    kept = np.delete(links, [1, 5])
    assert pa.links().tobytes() == kept.tobytes(), "the others keep their order"
    ul.run_twins(pa, ul.twin(state, lists(pins=pins, links=kept)), 5, "remove_links")
    assert pa.pin_schedule_builds() == builds + 1


def test_remove_bodies_through_a_rope(built_lib):
    pa = _mixed_world()
    for _ in range(8):
        pa.Update(DT, ul.cfg())
    state, pins, links = pa.state(), pa.pins(), pa.links()
    removed = [12, 7]                                       # the body on the taut rope, and a body in the chain
    filtered = removal_spec.filter(state, removed)
    new = removal_spec.new_index(len(state[0]), removed)
    kept_pins, kept_links = ul.remapped(pins, new), ul.remapped(links, new)
    assert len(kept_links) == len(links) - 2 and len(kept_pins) == len(pins) - 1
    assert pa.remove_bodies(removed).tolist() == new.tolist()
    assert pa.links().tobytes() == kept_links.tobytes() and pa.pins().tobytes() == kept_pins.tobytes()
    pb = ul.twin(filtered[0], lists(pins=kept_pins, links=kept_links))
    ul.same(pa, pb, "right after the removal")
    ul.run_twins(pa, pb, 8, "the removal")


def test_remove_pins_in_a_mixed_world_shifts_the_units(oracle, built_lib):
    bodies, pin_rows, link_rows = _alternating_chain(10, top=(0.0, 300.0))
    pins, links = ul.pins(pin_rows), link_spec.make_links(link_rows)
    pw, ow = ul.worlds(ul.scene(bodies), lists(pins=pins, links=links))
    cfg = ul.cfg()
    for s in range(4):
        _step(oracle, pw, ow, cfg, lists(pins=pins, links=links))
        ul.check(pw, ow, lists(pins=pins, links=links), s)
    pw.remove_pins([1, 3])
    pins = np.delete(pins, [1, 3])
    for s in range(4, 8):
        sched, _ = _step(oracle, pw, ow, cfg, lists(pins=pins, links=links))
        ul.check(pw, ow, lists(pins=pins, links=links), s)
    assert len(sched["order"]) == len(pins) + len(links) and pw.pin_schedule_builds() == 2


def test_length_and_anchor_edits_keep_the_schedule(oracle, built_lib):
    """a slack rope shortened below its current length engages at the next step; a spring's world anchor moves"""
    bodies = [(0.0, 100.0, 2.0, 2.0, False), (50.0, 100.0, 2.0, 2.0, False)]
    links = link_spec.make_links([(0, -1, (0.0, 0.0), (0.0, 120.0), 0.0, 60.0), (1, -1, (0.0, 0.0), (50.0, 110.0), 10.0, 10.0, 2.0, 0.5)])
    pw, ow = ul.worlds(ul.scene(bodies), lists(links=links))
    cfg = ul.cfg()
    for s in range(3):
        _, work = _step(oracle, pw, ow, cfg, lists(links=links))
        ul.check(pw, ow, lists(links=links), s)
        assert work[0].idle
    builds = pw.pin_schedule_builds()
    pw.set_link_lengths([0], np.array([[0.0, 15.0]], dtype=np.float32))
    links["min_length"][0], links["max_length"][0] = 0.0, 15.0
    pw.set_link_anchors([1], np.array([[0.0, 1.0, 55.0, 112.0]], dtype=np.float32))
    links["anchor1"][1], links["anchor2"][1] = (0.0, 1.0), (55.0, 112.0)
    assert pw.links().tobytes() == links.tobytes()
    for s in range(3, 6):
        _, work = _step(oracle, pw, ow, cfg, lists(links=links))
        ul.check(pw, ow, lists(links=links), s)
        assert work[0].active, "the shortened rope is taut"
        pulled = links["impulse"][0] < 0 if s == 3 else pulled
    assert pulled, "the rope pulled at the step after the edit"
    assert pw.pin_schedule_builds() == builds == 1


def test_edits_before_the_first_step_are_host_staged(built_lib):
    pa, pb = _mixed_world(), _mixed_world()
    links = pa.links()
    pa.set_link_lengths([6, 3], np.array([[0.0, 5.0], [1.0, 3.0]], dtype=np.float32))      # a shorter rope; a rod becomes limits
    pa.set_link_anchors([0], np.array([[-3.0, 0.5, 4.0, 0.0]], dtype=np.float32))
    links["max_length"][6] = 5.0
    links["min_length"][3], links["max_length"][3] = 1.0, 3.0
    links["anchor1"][0], links["anchor2"][0] = (-3.0, 0.5), (4.0, 0.0)
    assert pa.links().tobytes() == links.tobytes()
    pb.remove_links(list(range(len(links))))
    pb.add_links(links)
    ul.run_twins(pa, pb, 4, "host-staged edits")


def test_save_load_and_fork(built_lib):
    cfg = ul.cfg()
    pw = _mixed_world()
    for _ in range(6):
        pw.Update(DT, cfg)
    snap = pw.save()
    saved = (pw.pins().tobytes(), pw.links().tobytes())
    assert np.abs(pw.links()["impulse"]).max() > 0
    first = []
    for _ in range(8):
        pw.Update(DT, cfg)
        first.append((pw.bodies.tobytes(), pw.pins().tobytes(), pw.links().tobytes()))
    other = phyx_amd.World(0, gravity=G)
    other.load(snap)
    pw.load(snap)
    assert (pw.pins().tobytes(), pw.links().tobytes()) == saved == (other.pins().tobytes(), other.links().tobytes())
    for s in range(8):
        pw.Update(DT, cfg)
        other.Update(DT, cfg)
        assert (pw.bodies.tobytes(), pw.pins().tobytes(), pw.links().tobytes()) == first[s], "the loaded world differs at step %d" % s
        assert (other.bodies.tobytes(), other.pins().tobytes(), other.links().tobytes()) == first[s], "the fork differs at step %d" % s


# ---- the refusals ----
GOOD = (0, 1, (1.0, 0.0), (0.0, 1.0), 2.0, 3.0, 0.0, 0.0, 0.0, 0)


def _bad(**fields):
    p = np.array([GOOD, GOOD], dtype=link_dtype)
    for f, v in fields.items():
        if isinstance(v, tuple):
            p[f][1][v[0]] = v[1]
        else:
            p[f][1] = v
    return p


@pytest.mark.parametrize("staged", ["host", "device"])
def test_rejections_leave_the_world_unchanged(built_lib, staged):
    cfg = ul.cfg()
    pw = _mixed_world()
    if staged == "device":
        pw.Update(DT, cfg)
    n = pw.counts()[0]
    before = ul.snapshot_of(pw)
    bad = [dict(body1=-1), dict(body1=n), dict(body2=n), dict(body2=-2), dict(body1=2, body2=2),
           dict(anchor1=(1, np.nan)), dict(anchor2=(0, np.inf)), dict(min_length=np.nan), dict(max_length=np.inf), dict(hertz=np.nan),
           dict(damping_ratio=-np.inf), dict(impulse=np.nan),
           dict(min_length=-1.0), dict(min_length=4.0), dict(hertz=-1.0), dict(damping_ratio=-0.5),
           dict(hertz=2.0), dict(reserved=1)]
    for fields in bad:
        assert ul.raw_add(pw, KINDS[LINK], _bad(**fields)) == ERR_INVALID, fields
        ul.unchanged(pw, before)
    assert ul.raw_add(pw, KINDS[LINK], _bad(hertz=2.0, max_length=2.0)) == 0, "a spring with min == max is fine"
    pw.remove_links([pw.link_count() - 1, pw.link_count() - 2])
    before = ul.snapshot_of(pw)
    one = np.array([GOOD], dtype=link_dtype)
    assert ul.raw_add(pw, KINDS[LINK], one, count=-1) == ERR_INVALID
    assert ul.raw_add(pw, KINDS[LINK], one, null=True) == ERR_INVALID
    assert ul.raw_add(pw, KINDS[LINK], np.zeros(0, dtype=link_dtype), count=0, null=True) == 0, "an empty call is a true no-op"
    ul.unchanged(pw, before)
    nl = pw.link_count()
    for which in ([nl], [-1], [1, 1]):
        for call in (lambda: pw.remove_links(which), lambda: pw.set_link_anchors(which, np.zeros((len(which), 4), dtype=np.float32)),
                     lambda: pw.set_link_lengths(which, np.ones((len(which), 2), dtype=np.float32))):
            with pytest.raises(PhxError) as e:
                call()
            assert e.value.status == ERR_INVALID
            ul.unchanged(pw, before)
    spring = int(np.flatnonzero(pw.links()["hertz"] > 0)[0])
    for which, lengths in (([0], [1.0, np.nan]), ([0], [-1.0, 2.0]), ([0], [3.0, 2.0]), ([spring], [1.0, 2.0])):
        with pytest.raises(PhxError) as e:
            pw.set_link_lengths(which, np.array([lengths], dtype=np.float32))
        assert e.value.status == ERR_INVALID, lengths
        ul.unchanged(pw, before)
    with pytest.raises(PhxError) as e:
        pw.set_link_anchors([0], np.array([[0.0, np.nan, 0.0, 0.0]], dtype=np.float32))
    assert e.value.status == ERR_INVALID
    idx = np.zeros(1, dtype=np.int32)
    assert pw.L.phx_world_remove_links(pw.h, None, 1) == ERR_INVALID
    assert pw.L.phx_world_remove_links(pw.h, idx.ctypes.data_as(C.c_void_p), -1) == ERR_INVALID
    assert pw.L.phx_world_set_link_anchors(pw.h, idx.ctypes.data_as(C.c_void_p), None, 1) == ERR_INVALID
    assert pw.L.phx_world_set_link_lengths(pw.h, idx.ctypes.data_as(C.c_void_p), None, 1) == ERR_INVALID
    pw.remove_links([]); pw.set_link_anchors([], np.zeros((0, 4), dtype=np.float32)); pw.set_link_lengths([], np.zeros((0, 2), dtype=np.float32))
    ul.unchanged(pw, before)
    # inside a step every call is refused
    pw.PreSolve(DT)
    for call in (lambda: pw.add_links(one), lambda: pw.remove_links([0]), lambda: pw.set_link_anchors([0], np.zeros((1, 4), dtype=np.float32)),
                 lambda: pw.set_link_lengths([0], np.ones((1, 2), dtype=np.float32))):
        with pytest.raises(PhxError) as e:
            call()
        assert e.value.status == ERR_STATE
    pw.FinishStep(DT, cfg)
    assert pw.link_count() == nl
