"""Links on the device (include/phyx_amd.h LINKS) held to their specification, tests/link_spec.py: the device World and the oracle
World in lockstep, the spec's pass over pins and links applied to the oracle's bodies between its pre_solve and its solve on the
device's own schedule of units, every byte of the state, of the pins and of the links compared after every step; then the schedule's
paths, the life cycle by twins, and the refusals.  (The lockstep is that of tests/test_pins_gpu.py, copied.)"""
import ctypes as C

import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration, PhxError, scenes
from phyx_amd.api import link_dtype, pin_dtype
from helpers import oracle_world
from spawn_lockstep import compare
import link_spec
import removal_spec

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
NAMES = ("bodies", "manifolds", "contact points", "joints")
MODES = {"single": phyx_amd.ISLAND_SINGLE, "multiple_sloppy": phyx_amd.ISLAND_MULTIPLE_SLOPPY}
ERR_INVALID, ERR_STATE = -1, -5
NO_PINS = np.zeros(0, dtype=pin_dtype)


def _cfg(mode=phyx_amd.ISLAND_MULTIPLE_SLOPPY, iters=15):
    return Configuration(phyx_amd.SOLVE_AVX2, mode, iters, iters)


def _scene(rows):
    """rows (px, py, half_x, half_y, static) -> a scenes.py dict"""
    r = np.asarray([(a, b, c, d) for a, b, c, d, _ in rows], dtype=np.float32).reshape(-1, 4)
    return {"px": r[:, 0].copy(), "py": r[:, 1].copy(), "angle": np.zeros(len(rows), dtype=np.float32), "sx": r[:, 2].copy(), "sy": r[:, 3].copy(),
            "static": np.asarray([bool(s) for *_, s in rows], dtype=bool)}


def _pins(rows):
    p = np.zeros(len(rows), dtype=pin_dtype)
    for k, (a, b, a1, a2) in enumerate(rows):
        p[k] = (a, b, a1, a2, (0.0, 0.0))
    return p


def _worlds(scene, pins, links, gravity=G, with_oracle=True):
    pw = phyx_amd.World(0, gravity=gravity)
    pw.add_scene(scene)
    assert pw.add_pins(pins).tolist() == list(range(len(pins)))
    assert pw.add_links(links).tolist() == list(range(len(links)))
    return pw, (oracle_world(scene, gravity) if with_oracle else None)


def _step(oracle, pw, ow, cfg, pins, links, dt=DT):
    """1. pw.Update  2. ow.pre_solve  3. link_spec.solve_units on ow.bodies() on the device's own schedule of units  4. the oracle's
    solver on the device's contact schedule  5. ow.integrate_position.  `pins`, `links` are the spec's own lists.
    -> (the schedule, the links' prestep records)"""
    sched = pw.pin_schedule()
    assert sorted(sched["order"].tolist()) == list(range(len(pins) + len(links)))
    pw.Update(dt, cfg)
    ow.pre_solve(dt)
    work = link_spec.solve_units(ow.bodies(), pins, links, sched["order"], dt, pw.pin_iterations)
    order, offs = pw.solver.schedule()
    groups, _ = pw.solver.groups()
    b, cp, j = ow.bodies(), ow.contact_points(), ow.joints()
    assert len(order) == len(j)
    oracle.solver_solve_grouped(b, cp, j, order, offs, groups, cfg.contactIterationsCount, cfg.penetrationIterationsCount, oracle.STAG_COLOUR_SYNC)
    ow.integrate_position(dt)
    return sched, work


def _check(pw, ow, pins, links, s):
    compare(pw, ow, s)
    assert pw.pins().tobytes() == pins.tobytes(), "pins differ at step %d" % s
    assert pw.links().tobytes() == links.tobytes(), "links differ at step %d" % s


def _lockstep(oracle, pw, ow, cfg, pins, links, steps):
    """-> (the last schedule, per step the links' states)"""
    states = []
    for s in range(steps):
        sched, work = _step(oracle, pw, ow, cfg, pins, links)
        _check(pw, ow, pins, links, s)
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
    pw, ow = _worlds(_scene(bodies), NO_PINS, links)
    assert pw.link_count() == 1 and pw.pin_count() == 0
    assert pw.links().tobytes() == links.tobytes(), "before the first step the links wait on the host"
    sched, states = _lockstep(oracle, pw, ow, _cfg(), NO_PINS, links, 60)
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
    pins, links = _pins(pin_rows), link_spec.make_links(link_rows)
    pw, ow = _worlds(_scene(rows), pins, links)
    touched, rope = False, set()
    for s in range(40):
        sched, work = _step(oracle, pw, ow, _cfg(MODES[mode]), pins, links)
        _check(pw, ow, pins, links, s)
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


def _alternating_chain(units, top=(0.0, 500.0), spacing=10.0):
    """`units` boxes level with `top`; joints alternate pin / rod: a pin holds the neighbours' ends together, a rod of 2 joins points
    that lie 2 apart"""
    h = spacing / 2.0
    bodies = [(top[0] + spacing * (k + 0.5), top[1], 3.0, 1.0, False) for k in range(units)]
    pins, links = [(0, -1, (-h, 0.0), top)], []
    for k in range(1, units):
        if k % 2:
            links += [(k, k - 1, (-h + 1.0, 0.0), (h - 1.0, 0.0), 2.0, 2.0)]
        else:
            pins += [(k, k - 1, (-h, 0.0), (h, 0.0))]
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
    pins, links = _pins(pin_rows), link_spec.make_links(link_rows)
    pw, ow = _worlds(_scene(bodies), pins, links)
    sched, _ = _lockstep(oracle, pw, ow, _cfg(), pins, links, steps)
    assert sched["lds_groups"] == lds and len(sched["group_offsets"]) - 1 == groups
    if case != "pairs300_cap64":
        assert len(sched["class_offsets"]) - 1 == 2, "a chain needs two classes"
    assert np.abs(pins["impulse"]).max() > 0 and np.abs(links["impulse"]).max() > 0


# ---- the life cycle, by twins ----
def _same(a, b, what):
    assert a.counts() == b.counts(), "counts differ %s" % what
    for name, x, y in zip(NAMES, a.state(), b.state()):
        assert x.tobytes() == y.tobytes(), "%s differ %s" % (name, what)
    assert a.pins().tobytes() == b.pins().tobytes(), "pins differ %s" % what
    assert a.links().tobytes() == b.links().tobytes(), "links differ %s" % what


def _mixed_world():
    """a 10-unit alternating chain, a pair on a spring, a body on a taut rope from the chain's body 4 and one on a slack rope"""
    bodies, pin_rows, link_rows = _alternating_chain(10, top=(0.0, 300.0))
    bodies += [(-100.0, 300.0, 4.0, 1.5, False), (-85.0, 300.0, 4.0, 1.5, False)]
    link_rows += [(10, 11, (4.0, 0.0), (-4.0, 0.0), 5.0, 5.0, 2.0, 0.2)]
    bodies += [(45.0, 280.0, 2.0, 2.0, False), (200.0, 300.0, 2.0, 2.0, False)]
    link_rows += [(12, 4, (0.0, 2.0), (0.0, -1.0), 0.0, 10.0), (13, -1, (0.0, 0.0), (200.0, 320.0), 0.0, 60.0)]
    pw, _ = _worlds(_scene(bodies), _pins(pin_rows), link_spec.make_links(link_rows), with_oracle=False)
    return pw


def _twin(state, pins, links):
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*state)
    pb.add_pins(pins)
    pb.add_links(links)
    return pb


def _run_twins(pa, pb, steps, what):
    cfg = _cfg()
    for s in range(steps):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "at step %d after %s" % (s, what))


def test_remove_links(built_lib):
    pa = _mixed_world()
    for _ in range(5):
        pa.Update(DT, _cfg())
    state, pins, links = pa.state(), pa.pins(), pa.links()
    builds = pa.pin_schedule_builds()
    assert np.abs(links["impulse"]).max() > 0
    pa.remove_links([5, 1])
    kept = np.delete(links, [1, 5])
    assert pa.links().tobytes() == kept.tobytes(), "the others keep their order"
    _run_twins(pa, _twin(state, pins, kept), 5, "remove_links")
    assert pa.pin_schedule_builds() == builds + 1


def test_remove_bodies_through_a_rope(built_lib):
    pa = _mixed_world()
    for _ in range(8):
        pa.Update(DT, _cfg())
    state, pins, links = pa.state(), pa.pins(), pa.links()
    removed = [12, 7]                                       # the body on the taut rope, and a body in the chain
    filtered = removal_spec.filter(state, removed)
    new = removal_spec.new_index(len(state[0]), removed)

    def remapped(units):
        keep = np.array([new[p["body1"]] >= 0 and (p["body2"] < 0 or new[p["body2"]] >= 0) for p in units], dtype=bool)
        kept = units[keep].copy()
        kept["body1"] = new[kept["body1"]]
        kept["body2"] = np.where(kept["body2"] < 0, -1, new[np.maximum(kept["body2"], 0)])
        return kept

    kept_pins, kept_links = remapped(pins), remapped(links)
    assert len(kept_links) == len(links) - 2 and len(kept_pins) == len(pins) - 1
    assert pa.remove_bodies(removed).tolist() == new.tolist()
    assert pa.links().tobytes() == kept_links.tobytes() and pa.pins().tobytes() == kept_pins.tobytes()
    pb = _twin(filtered[0], kept_pins, kept_links)
    _same(pa, pb, "right after the removal")
    _run_twins(pa, pb, 8, "the removal")


def test_remove_pins_in_a_mixed_world_shifts_the_units(oracle, built_lib):
    bodies, pin_rows, link_rows = _alternating_chain(10, top=(0.0, 300.0))
    pins, links = _pins(pin_rows), link_spec.make_links(link_rows)
    pw, ow = _worlds(_scene(bodies), pins, links)
    cfg = _cfg()
    for s in range(4):
        _step(oracle, pw, ow, cfg, pins, links)
        _check(pw, ow, pins, links, s)
    pw.remove_pins([1, 3])
    pins = np.delete(pins, [1, 3])
    for s in range(4, 8):
        sched, _ = _step(oracle, pw, ow, cfg, pins, links)
        _check(pw, ow, pins, links, s)
    assert len(sched["order"]) == len(pins) + len(links) and pw.pin_schedule_builds() == 2


def test_length_and_anchor_edits_keep_the_schedule(oracle, built_lib):
    """a slack rope shortened below its current length engages at the next step; a spring's world anchor moves"""
    bodies = [(0.0, 100.0, 2.0, 2.0, False), (50.0, 100.0, 2.0, 2.0, False)]
    links = link_spec.make_links([(0, -1, (0.0, 0.0), (0.0, 120.0), 0.0, 60.0), (1, -1, (0.0, 0.0), (50.0, 110.0), 10.0, 10.0, 2.0, 0.5)])
    pw, ow = _worlds(_scene(bodies), NO_PINS, links)
    cfg = _cfg()
    for s in range(3):
        _, work = _step(oracle, pw, ow, cfg, NO_PINS, links)
        _check(pw, ow, NO_PINS, links, s)
        assert work[0].idle
    builds = pw.pin_schedule_builds()
    pw.set_link_lengths([0], np.array([[0.0, 15.0]], dtype=np.float32))
    links["min_length"][0], links["max_length"][0] = 0.0, 15.0
    pw.set_link_anchors([1], np.array([[0.0, 1.0, 55.0, 112.0]], dtype=np.float32))
    links["anchor1"][1], links["anchor2"][1] = (0.0, 1.0), (55.0, 112.0)
    assert pw.links().tobytes() == links.tobytes()
    for s in range(3, 6):
        _, work = _step(oracle, pw, ow, cfg, NO_PINS, links)
        _check(pw, ow, NO_PINS, links, s)
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
    _run_twins(pa, pb, 4, "host-staged edits")


def test_save_load_and_fork(built_lib):
    cfg = _cfg()
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


def test_a_snapshot_with_links_has_no_blob(built_lib):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scenes.stack(2, 3))
    pw.add_links(link_spec.make_links([(1, -1, (0.0, 0.0), (0.0, 90.0), 0.0, 80.0)]))
    snap = pw.save()
    with pytest.raises(PhxError) as e:
        snap.to_bytes()
    assert e.value.status == ERR_STATE and "links" in str(e.value)
    n = C.c_size_t(0)
    assert pw.L.phx_snapshot_blob_bytes(snap.h, C.byref(n)) == ERR_STATE
    pw.remove_links([0])
    assert len(pw.save().to_bytes()) > 0


def test_set_state_leaves_no_link(built_lib):
    pw = _mixed_world()
    pw.Update(DT, _cfg())
    pw.set_state(*pw.state())
    assert pw.link_count() == 0 and len(pw.links()) == 0 and pw.pin_count() == 0
    pw.Update(DT, _cfg())


def test_a_world_that_lost_its_links_is_a_world_without(built_lib):
    cfg = _cfg()
    sc = scenes.stack(3, 6)
    pa, pb = phyx_amd.World(0, gravity=G), phyx_amd.World(0, gravity=G)
    pa.add_scene(sc); pb.add_scene(sc)
    pa.add_links(link_spec.make_links([(1, 2, (0.0, 5.0), (0.0, -5.0), 1.0, 1.0), (3, -1, (0.0, 0.0), (0.0, 50.0), 0.0, 10.0)]))
    pa.remove_links([0, 1])
    assert pa.link_count() == 0
    for s in range(10):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        for name, x, y in zip(NAMES, pa.state(), pb.state()):
            assert x.tobytes() == y.tobytes(), "%s differ at step %d" % (name, s)
    assert pa.pin_schedule_builds() == 0, "no pins and no links: no schedule, no pass"
    assert pa.save().to_bytes() == pb.save().to_bytes(), "a snapshot without links is what it was"


# ---- the refusals ----
def _unchanged(pw, before):
    bodies, pins, links, builds = before
    assert pw.bodies.tobytes() == bodies and pw.pins().tobytes() == pins and pw.links().tobytes() == links and pw.pin_schedule_builds() == builds


def _raw_add(pw, links, count=None, null=False):
    p = np.ascontiguousarray(links, dtype=link_dtype)
    return pw.L.phx_world_add_links(pw.h, None if null else p.ctypes.data_as(C.c_void_p), len(p) if count is None else count, None)


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
    cfg = _cfg()
    pw = _mixed_world()
    if staged == "device":
        pw.Update(DT, cfg)
    n = pw.counts()[0]
    before = (pw.bodies.tobytes(), pw.pins().tobytes(), pw.links().tobytes(), pw.pin_schedule_builds())
    bad = [dict(body1=-1), dict(body1=n), dict(body2=n), dict(body2=-2), dict(body1=2, body2=2),
           dict(anchor1=(1, np.nan)), dict(anchor2=(0, np.inf)), dict(min_length=np.nan), dict(max_length=np.inf), dict(hertz=np.nan),
           dict(damping_ratio=-np.inf), dict(impulse=np.nan),
           dict(min_length=-1.0), dict(min_length=4.0), dict(hertz=-1.0), dict(damping_ratio=-0.5),
           dict(hertz=2.0), dict(reserved=1)]
    for fields in bad:
        assert _raw_add(pw, _bad(**fields)) == ERR_INVALID, fields
        _unchanged(pw, before)
    assert _raw_add(pw, _bad(hertz=2.0, max_length=2.0)) == 0, "a spring with min == max is fine"
    pw.remove_links([pw.link_count() - 1, pw.link_count() - 2])
    before = (pw.bodies.tobytes(), pw.pins().tobytes(), pw.links().tobytes(), pw.pin_schedule_builds())
    one = np.array([GOOD], dtype=link_dtype)
    assert _raw_add(pw, one, count=-1) == ERR_INVALID
    assert _raw_add(pw, one, null=True) == ERR_INVALID
    assert _raw_add(pw, np.zeros(0, dtype=link_dtype), count=0, null=True) == 0, "an empty call is a true no-op"
    _unchanged(pw, before)
    nl = pw.link_count()
    for which in ([nl], [-1], [1, 1]):
        for call in (lambda: pw.remove_links(which), lambda: pw.set_link_anchors(which, np.zeros((len(which), 4), dtype=np.float32)),
                     lambda: pw.set_link_lengths(which, np.ones((len(which), 2), dtype=np.float32))):
            with pytest.raises(PhxError) as e:
                call()
            assert e.value.status == ERR_INVALID
            _unchanged(pw, before)
    spring = int(np.flatnonzero(pw.links()["hertz"] > 0)[0])
    for which, lengths in (([0], [1.0, np.nan]), ([0], [-1.0, 2.0]), ([0], [3.0, 2.0]), ([spring], [1.0, 2.0])):
        with pytest.raises(PhxError) as e:
            pw.set_link_lengths(which, np.array([lengths], dtype=np.float32))
        assert e.value.status == ERR_INVALID, lengths
        _unchanged(pw, before)
    with pytest.raises(PhxError) as e:
        pw.set_link_anchors([0], np.array([[0.0, np.nan, 0.0, 0.0]], dtype=np.float32))
    assert e.value.status == ERR_INVALID
    idx = np.zeros(1, dtype=np.int32)
    assert pw.L.phx_world_remove_links(pw.h, None, 1) == ERR_INVALID
    assert pw.L.phx_world_remove_links(pw.h, idx.ctypes.data_as(C.c_void_p), -1) == ERR_INVALID
    assert pw.L.phx_world_set_link_anchors(pw.h, idx.ctypes.data_as(C.c_void_p), None, 1) == ERR_INVALID
    assert pw.L.phx_world_set_link_lengths(pw.h, idx.ctypes.data_as(C.c_void_p), None, 1) == ERR_INVALID
    pw.remove_links([]); pw.set_link_anchors([], np.zeros((0, 4), dtype=np.float32)); pw.set_link_lengths([], np.zeros((0, 2), dtype=np.float32))
    _unchanged(pw, before)
    # inside a step every call is refused
    pw.PreSolve(DT)
    for call in (lambda: pw.add_links(one), lambda: pw.remove_links([0]), lambda: pw.set_link_anchors([0], np.zeros((1, 4), dtype=np.float32)),
                 lambda: pw.set_link_lengths([0], np.ones((1, 2), dtype=np.float32))):
        with pytest.raises(PhxError) as e:
            call()
        assert e.value.status == ERR_STATE
    pw.FinishStep(DT, cfg)
    assert pw.link_count() == nl


def test_sharded_worlds_carry_no_links(built_lib):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scenes.stack(2, 3))
    rope = link_spec.make_links([(1, -1, (0.0, 0.0), (0.0, 90.0), 0.0, 80.0)])
    pw.add_links(rope)
    with pytest.raises(PhxError) as e:
        pw.set_shard(0, 2)
    assert e.value.status == ERR_STATE and "links" in str(e.value)
    n = pw.counts()[0]
    with pytest.raises(PhxError) as e:
        pw.reslab(np.arange(n, dtype=np.int64), n, (-1e9, 1e9))
    assert e.value.status == ERR_STATE and "links" in str(e.value)
    pw.set_shard(0, 1)
    sharded = phyx_amd.World(0, gravity=G)
    sharded.add_scene(scenes.stack(2, 3))
    sharded.set_shard(0, 2)
    with pytest.raises(PhxError) as e:
        sharded.add_links(rope)
    assert e.value.status == ERR_STATE and sharded.link_count() == 0


def test_set_comm_refuses_a_world_with_links(built_lib):
    """as tests/test_pins_gpu.py: in a child process, so that RCCL's bootstrap cannot hang the suite's"""
    import os
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "links_comm_worker.py")
    env = dict(os.environ, PHX_COMM_TIMEOUT_S="60")
    for attempt in range(2):
        p = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=300)
        if "NO COMMUNICATOR" not in p.stdout:
            break
    if "NO COMMUNICATOR" in p.stdout:
        pytest.skip("no RCCL communicator on this box: " + p.stdout[-300:])
    assert p.returncode == 0 and "links comm worker ok" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]
