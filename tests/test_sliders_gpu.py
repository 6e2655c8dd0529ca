"""Sliders on the device (include/phyx_amd.h SLIDERS) held to their specification, tests/slider_spec.py, in the lockstep of
tests/unit_lockstep.py; then the schedule's paths, the life cycle by twins, and the refusals.  (What every kind of unit has alike is in
tests/test_units_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import phyx_amd
from phyx_amd import PhxError
from phyx_amd.api import slider_dtype
import angle_spec
import removal_spec
from slider_corpus import state_of as _state
import slider_spec
import unit_lockstep as ul
from unit_lockstep import DT, G, MODES, ERR_INVALID, ERR_CAPACITY, ERR_STATE, O, X, Y, lists
from unit_scenes import MIXED, mixed_chain as _mixed_chain, mixed_world
from unit_spec import KINDS, SLIDER

pytestmark = pytest.mark.gpu


def _step(oracle, pw, ow, cfg, units):
    """-> (the schedule, the sliders' prestep records)"""
    sched, work = ul.step(oracle, pw, ow, cfg, units)
    return sched, work[SLIDER]


def _lockstep(oracle, pw, ow, cfg, units, steps, first=0):
    """-> (the last schedule, per step the sliders' states as tests/slider_corpus.py names them)"""
    states = []
    for s in range(first, first + steps):
        sched, work = _step(oracle, pw, ow, cfg, units)
        ul.check(pw, ow, units, s)
        states.append([_state(w) for w in work])
    return sched, states


# ---- one body on one world slider ----
@pytest.mark.parametrize("kind", ["lock", "limit", "spring", "motor"])
def test_one_body_on_a_world_slider(oracle, built_lib, kind):
    body = [(0.0, 100.0, 3.0, 1.0, False, 0.4)]
    slider = {"lock": (0, -1, (1.0, 0.5), (0.0, 100.0), (1.0, 0.5), 2.0, 2.0),
              "limit": (0, -1, O, (0.0, 100.0), Y, -5.0, 5.0),                      # it falls 5 in 13 steps
              "spring": (0, -1, O, (0.0, 100.0), Y, 0.0, 0.0, 2.0, 0.3),
              "motor": (0, -1, O, (0.0, 100.0), X, -1.0e5, 1.0e5, 0.0, 0.0, 1000.0, 1.0e-3)}[kind]      # (weak: still accelerating, its impulse at the clamp, after 60 steps)
    sliders = slider_spec.make_sliders([slider])
    pw, ow = ul.worlds(ul.scene(body), lists(sliders=sliders))
    assert pw.slider_count() == 1 and pw.pin_count() == 0 and pw.link_count() == 0 and pw.angle_count() == 0
    assert pw.sliders().tobytes() == sliders.tobytes(), "before the first step the sliders wait on the host"
    sched, states = _lockstep(oracle, pw, ow, ul.cfg(), lists(sliders=sliders), 60)
    assert sched["lds_groups"] == 1 and len(sched["class_offsets"]) == 2
    flat = [s[0] for s in states]
    if kind in ("lock", "motor"):
        assert sliders["impulse"][0] != 0, "row P carries the weight across the rail"
    if kind == "limit":
        first = flat.index("PL")
        assert first > 10 and set(flat[:first]) == {"P-idle"} and set(flat[first:]) == {"PL"}, "the limit was idle, then engaged"
        assert sliders["axis_impulse"][0] >= 0
    elif kind == "motor":
        assert set(flat) == {"PM-idle"} and sliders["motor_impulse"][0] == np.float32(1.0e-3) * np.float32(DT) and sliders["axis_impulse"][0] == 0
    else:
        assert set(flat) == {"PL"} and sliders["axis_impulse"][0] != 0
    assert pw.pin_schedule_builds() == 1


# ---- among contacts ----
@pytest.mark.parametrize("mode", list(MODES))
def test_a_limited_slider_among_contacts(oracle, built_lib, mode):
    """a platform on a vertical world rail falls to its lower stop and a box lands on it there"""
    rows = [(0.0, 20.0, 4.0, 1.0, False), (0.5, 26.0, 2.0, 2.0, False)]
    sliders = slider_spec.make_sliders([(0, -1, O, (0.0, 20.0), Y, -5.0, 5.0)])
    pw, ow = ul.worlds(ul.scene(rows), lists(sliders=sliders))
    touched, seen = False, set()
    for s in range(60):
        _, work = _step(oracle, pw, ow, ul.cfg(MODES[mode]), lists(sliders=sliders))
        ul.check(pw, ow, lists(sliders=sliders), s)
        seen.add(_state(work[0]))
        touched = touched or len(pw.manifolds) > 0
    assert pw.pin_schedule_builds() == 1
    assert touched, "the box never landed on the platform"
    assert seen == {"P-idle", "PL"}, "the platform fell freely, then stood on its stop"
    assert sliders["axis_impulse"][0] > 0, "the stop carries the platform and the box"


# ---- the paths ----
@pytest.mark.parametrize("case", ["chain20_cap16", "chain20_pairs_cap16", "chain20", "chain65", "chain130"])
def test_the_paths(oracle, built_lib, monkeypatch, case):
    """40 units in one component above a cap of 16: the trailing group alone; the same chain beside 20 pairs of a slider and a lock at
    cap 16: several LDS groups and the trailing group in one pass; the chain at the default: one LDS group; 130 units at the default: one
    LDS group of three waves; 260 units in one component, more than a workgroup: the HBM path at the default"""
    if case in ("chain20_cap16", "chain20_pairs_cap16"):
        monkeypatch.setenv("PHX_PIN_GROUP_PINS", "16")
    bodies, (pins, links, angles, sliders) = _mixed_chain({"chain65": 65, "chain130": 130}.get(case, 20))
    if case == "chain20_pairs_cap16":
        first, slider_rows, angle_rows = len(bodies), [], []
        for k in range(20):
            a = first + 2 * k
            bodies += [(40.0 * k, 300.0, 4.0, 1.5, False, 0.1 * (k % 5)), (40.0 * k + 10.0, 300.0, 4.0, 2.0, False)]
            slider_rows += [(a + 1, a, (-5.0, 0.0), (5.0, 0.0), (1.0, 0.1 * (k % 3)), -0.5, 0.5, 0.0, 0.0, 1.0, 1.0e-4 * (k % 2))]
            angle_rows += [(a + 1, a, 0.0, 0.0)]
        sliders, angles = np.concatenate([sliders, slider_spec.make_sliders(slider_rows)]), np.concatenate([angles, angle_spec.make_angles(angle_rows)])
    pw, ow = ul.worlds(ul.scene(bodies), [pins, links, angles, sliders])
    steps = 4 if case in ("chain65", "chain130") else 14
    sched, states = _lockstep(oracle, pw, ow, ul.cfg(), [pins, links, angles, sliders], steps)
    lds, groups = sched["lds_groups"], len(sched["group_offsets"]) - 1
    if case in ("chain20", "chain65"):
        assert (lds, groups) == (1, 1)
    elif case == "chain20_pairs_cap16":
        assert lds >= 2 and groups == lds + 1, "the pairs in LDS groups, the chain in the trailing group"
    else:
        assert (lds, groups) == (0, 1), "one component that no workgroup takes"
    assert len(sched["order"]) == len(pins) + len(links) + len(angles) + len(sliders) == (2 * len(bodies) if "pairs" not in case else 80)
    assert np.abs(pins["impulse"]).max() > 0 and np.abs(links["impulse"]).max() > 0 and np.abs(angles["impulse"]).max() > 0
    assert np.abs(sliders["impulse"]).max() > 0
    if case not in ("chain65", "chain130"):
        assert "PL" in {r for s in states for r in s} and np.abs(sliders["axis_impulse"]).max() > 0, "no telescope of the falling chain reached a stop"


def test_a_world_with_sliders_only(oracle, built_lib):
    bodies = [(30.0 * k, 100.0, 3.0, 1.0, False, 0.2 * k) for k in range(6)]
    sliders = slider_spec.make_sliders([(1, 0, O, O, X, 30.0, 30.0), (2, 1, (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), 10.0, 30.0), (3, 2, O, O, X, 30.0, 30.0, 1.5, 0.2),
                                        (4, 3, O, O, X, -900.0, 900.0, 0.0, 0.0, 2.0, 1.0e-4), (5, -1, O, (150.0, 100.0), Y, 0.0, 0.0)])
    pw, ow = ul.worlds(ul.scene(bodies), lists(sliders=sliders))
    pw.set_velocities([0], np.array([[5.0, 0.0, 1.5]], dtype=np.float32))
    b = ow.bodies()
    b["velocity"]["x"][0], b["angular_velocity"][0] = 5.0, 1.5
    sched, states = _lockstep(oracle, pw, ow, ul.cfg(), lists(sliders=sliders), 12)
    assert pw.pin_count() == 0 and pw.link_count() == 0 and pw.angle_count() == 0 and len(sched["order"]) == 5
    assert states[0] == ["PL", "P-idle", "PL", "PM-idle", "PL"]


# ---- the life cycle, by twins ----
def _mixed_world():
    return mixed_world("slider")


def test_remove_sliders(built_lib):
    pa = _mixed_world()
    for _ in range(8):
        pa.Update(DT, ul.cfg())
    state, (pins, links, angles, sliders) = pa.state(), ul.lists_of(pa)
    builds = pa.pin_schedule_builds()
    assert all(np.abs(sliders[f]).max() > 0 for f in ("impulse", "axis_impulse", "motor_impulse"))
    pa.remove_sliders([4, 1])
    kept = np.delete(sliders, [1, 4])
    assert pa.sliders().tobytes() == kept.tobytes(), "the others keep their order"
    ul.run_twins(pa, ul.twin(state, [pins, links, angles, kept]), 5, "remove_sliders")
    assert pa.pin_schedule_builds() == builds + 1


def test_removing_pins_links_and_angles_shifts_the_slider_units(oracle, built_lib):
    bodies, (pins, links, angles, sliders) = MIXED["slider"]()
    pw, ow = ul.worlds(ul.scene(bodies), [pins, links, angles, sliders])
    cfg = ul.cfg()
    _lockstep(oracle, pw, ow, cfg, [pins, links, angles, sliders], 4)
    pw.remove_pins([3, 5])
    pw.remove_links([0])
    pw.remove_angles([2])
    pins, links, angles = np.delete(pins, [3, 5]), np.delete(links, [0]), np.delete(angles, [2])
    sched, _ = _lockstep(oracle, pw, ow, cfg, [pins, links, angles, sliders], 4, first=4)
    assert len(sched["order"]) == len(pins) + len(links) + len(angles) + len(sliders) and pw.pin_schedule_builds() == 2


def test_remove_bodies_through_a_slider_chain(built_lib):
    pa = _mixed_world()
    for _ in range(8):
        pa.Update(DT, ul.cfg())
    state, units = pa.state(), ul.lists_of(pa)
    removed = [12, 4]                                       # the carriage on the world rail (the rail of the second), and a telescope's carriage
    filtered = removal_spec.filter(state, removed)
    new = removal_spec.new_index(len(state[0]), removed)
    kept = [ul.remapped(u, new) for u in units]
    assert len(kept[SLIDER]) == len(units[SLIDER]) - 3, "the telescope of body 4 and both sliders of body 12 went"
    assert pa.remove_bodies(removed).tolist() == new.tolist()
    assert [u.tobytes() for u in ul.lists_of(pa)] == [u.tobytes() for u in kept]
    pb = ul.twin(filtered[0], kept)
    ul.same(pa, pb, "right after the removal")
    ul.run_twins(pa, pb, 8, "the removal")


def test_limit_motor_and_anchor_edits_keep_the_schedule(oracle, built_lib):
    """on the device: free limits narrowed below the current translation engage at the next step; a motor is switched on, then
    reversed; an anchor is moved across the rail and row P pulls the carriage over"""
    bodies = [(0.0, 100.0, 3.0, 1.0, False, 0.3), (50.0, 100.0, 3.0, 1.0, False)]
    sliders = slider_spec.make_sliders([(0, -1, O, (-2.0, 100.0), X, -10.0, 10.0), (1, -1, O, (50.0, 100.0), X, -500.0, 500.0)])
    pw, ow = ul.worlds(ul.scene(bodies), lists(sliders=sliders), gravity=0.0)
    cfg = ul.cfg()
    _, states = _lockstep(oracle, pw, ow, cfg, lists(sliders=sliders), 3)
    assert states == [["P-idle", "P-idle"]] * 3
    builds = pw.pin_schedule_builds()
    pw.set_slider_limits([0], np.array([[-1.0, 1.0]], dtype=np.float32))                  # s = 2: past the new upper stop
    sliders["lower"][0], sliders["upper"][0] = -1.0, 1.0
    pw.set_slider_motors([1], np.array([[2.0, 1.0e-4]], dtype=np.float32))
    sliders["motor_speed"][1], sliders["max_force"][1] = 2.0, 1.0e-4
    assert pw.sliders().tobytes() == sliders.tobytes()
    _, states = _lockstep(oracle, pw, ow, cfg, lists(sliders=sliders), 1, first=3)
    assert states == [["PL", "PM-idle"]] and sliders["axis_impulse"][0] < 0, "the narrowed limit pushed back at the step after the edit"
    _lockstep(oracle, pw, ow, cfg, lists(sliders=sliders), 2, first=4)
    assert sliders["motor_impulse"][1] > 0
    pw.set_slider_motors([1, 0], np.array([[-2.0, 1.0e-4], [0.5, 2.0e-5]], dtype=np.float32))
    sliders["motor_speed"][1] = -2.0
    sliders["motor_speed"][0], sliders["max_force"][0] = 0.5, 2.0e-5
    pw.set_slider_anchors([1], np.array([[0.0, 0.0, 50.0, 101.0]], dtype=np.float32))
    sliders["anchor2"][1] = (50.0, 101.0)
    assert pw.sliders().tobytes() == sliders.tobytes()
    _, states = _lockstep(oracle, pw, ow, cfg, lists(sliders=sliders), 3, first=6)
    assert all(s[0] in ("PLM", "PM-idle") and s[1] == "PM-idle" for s in states)
    assert sliders["motor_impulse"][1] < 0 and sliders["impulse"][1] != 0
    assert pw.bodies["velocity"]["y"][1] > 0, "the rail moved up by 1 and row P pulls the carriage after it"
    assert pw.pin_schedule_builds() == builds == 1


def test_edits_before_the_first_step_are_host_staged(built_lib):
    pa, pb = _mixed_world(), _mixed_world()
    sliders = pa.sliders()
    pa.set_slider_limits([2, 4], np.array([[-0.05, 0.4], [-3.0, 3.0]], dtype=np.float32))
    pa.set_slider_motors([5, 0], np.array([[-3.0, 1.0e-4], [1.0, 2.0e-5]], dtype=np.float32))
    pa.set_slider_anchors([1], np.array([[-4.0, 0.5, 5.0, 0.0]], dtype=np.float32))
    sliders["lower"][2], sliders["upper"][2] = -0.05, 0.4
    sliders["lower"][4], sliders["upper"][4] = -3.0, 3.0
    sliders["motor_speed"][5], sliders["max_force"][5] = -3.0, 1.0e-4
    sliders["motor_speed"][0], sliders["max_force"][0] = 1.0, 2.0e-5
    sliders["anchor1"][1], sliders["anchor2"][1] = (-4.0, 0.5), (5.0, 0.0)
    assert pa.sliders().tobytes() == sliders.tobytes() and pa.pin_schedule_builds() == 0
    pb.remove_sliders(list(range(len(sliders))))
    pb.add_sliders(sliders)
    ul.run_twins(pa, pb, 4, "host-staged edits")
    assert pa.pin_schedule_builds() == 1


def test_save_load_and_fork(built_lib):
    cfg = ul.cfg()
    pw = _mixed_world()
    for _ in range(6):
        pw.Update(DT, cfg)
    snap = pw.save()

    def bytes_of(w):
        return tuple(u.tobytes() for u in ul.lists_of(w))

    saved = bytes_of(pw)
    assert all(np.abs(pw.sliders()[f]).max() > 0 for f in ("impulse", "axis_impulse", "motor_impulse"))
    first = []
    for _ in range(8):
        pw.Update(DT, cfg)
        first.append((pw.bodies.tobytes(),) + bytes_of(pw))
    other = phyx_amd.World(0, gravity=G)
    other.load(snap)
    pw.load(snap)
    assert bytes_of(pw) == saved == bytes_of(other)
    for s in range(8):
        pw.Update(DT, cfg)
        other.Update(DT, cfg)
        assert (pw.bodies.tobytes(),) + bytes_of(pw) == first[s], "the loaded world differs at step %d" % s
        assert (other.bodies.tobytes(),) + bytes_of(other) == first[s], "the fork differs at step %d" % s


def test_an_all_idle_slider_leaves_its_bodies_as_without_it(built_lib):
    """limits not reached, no motor, and a body that moves along its rail only: a box at rest, frame the identity, falls along a
    vertical world rail through its centre.  Row P is on, its C and its cdot are exactly 0, so its impulse is, and L and M are off: the
    body's bytes are those of the twin world that has no slider, on every step."""
    cfg = ul.cfg()
    rows = [(0.0, 500.0, 3.0, 1.0, False)]
    pa, pb = phyx_amd.World(0, gravity=G), phyx_amd.World(0, gravity=G)
    pa.add_scene(ul.scene(rows)); pb.add_scene(ul.scene(rows))
    pa.add_sliders([(0, -1, O, (0.0, 500.0), Y, -1.0e5, 1.0e5)])
    for s in range(20):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        assert pa.bodies.tobytes() == pb.bodies.tobytes(), "the idle slider changed a bit at step %d" % s
    got = pa.sliders()
    assert got["impulse"][0] == 0 and got["axis_impulse"][0] == 0 and got["motor_impulse"][0] == 0
    assert pa.bodies["velocity"]["y"][0] < -60 and pa.pin_schedule_builds() == 1


# ---- the refusals ----
GOOD = (0, 1, (0.0, 0.0), (0.0, 0.0), (1.0, 0.0), -0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0)


def _bad(**fields):
    p = np.array([GOOD, GOOD], dtype=slider_dtype)
    for f, v in fields.items():
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
    A = "phx_world_add_sliders: slider 1: "
    nan, inf = np.nan, np.inf
    bad = [(dict(body1=-1), A + "body1 -1 out of range [0, %d)" % n), (dict(body1=n), A + "body1 %d out of range [0, %d)" % (n, n)),
           (dict(body2=n), A + "body2 %d is neither -1 nor in [0, %d)" % (n, n)), (dict(body2=-2), A + "body2 -2 is neither -1 nor in [0, %d)" % n),
           (dict(body1=2, body2=2), A + "both ends on body 2"),
           (dict(anchor1=(nan, 0.0)), A + "value 0 is not finite"), (dict(anchor1=(0.0, inf)), A + "value 1 is not finite"),
           (dict(anchor2=(-inf, 0.0)), A + "value 2 is not finite"), (dict(anchor2=(0.0, nan)), A + "value 3 is not finite"),
           (dict(axis=(nan, 1.0)), A + "value 4 is not finite"), (dict(axis=(1.0, inf)), A + "value 5 is not finite"),
           (dict(lower=nan), A + "value 6 is not finite"), (dict(upper=inf), A + "value 7 is not finite"), (dict(hertz=nan), A + "value 8 is not finite"),
           (dict(damping_ratio=-inf), A + "value 9 is not finite"), (dict(motor_speed=inf), A + "value 10 is not finite"),
           (dict(max_force=nan), A + "value 11 is not finite"), (dict(impulse=nan), A + "value 12 is not finite"),
           (dict(axis_impulse=inf), A + "value 13 is not finite"), (dict(motor_impulse=-inf), A + "value 14 is not finite"),
           (dict(axis=(0.0, 0.0)), A + "axis (0, 0) is too short to give a direction"),
           (dict(axis=(2.0 ** -10, 0.0)), A + "axis (0.000976562, 0) is too short to give a direction"),
           (dict(hertz=-1.0), A + "negative hertz or damping_ratio"), (dict(damping_ratio=-0.5), A + "negative hertz or damping_ratio"),
           (dict(lower=1.0), A + "limits [1, 0.5] are not lower <= upper"),
           (dict(hertz=2.0), A + "a spring (hertz 2) needs lower == upper"),
           (dict(max_force=-1.0), A + "negative max_force -1"),
           (dict(reserved=7), A + "reserved must be 0")]
    for fields, message in bad:
        assert ul.raw_add(pw, KINDS[SLIDER], _bad(**fields)) == ERR_INVALID, fields
        assert ul.message(pw) == message
        ul.unchanged(pw, before)
    assert ul.raw_add(pw, KINDS[SLIDER], _bad(hertz=2.0, lower=0.5, axis=(0.0, 2.0 ** -9))) == 0, "a spring with lower == upper is fine, and so is an axis of 2^-9"
    pw.remove_sliders([pw.slider_count() - 1, pw.slider_count() - 2])
    before = ul.snapshot_of(pw)
    one = np.array([GOOD], dtype=slider_dtype)
    assert ul.raw_add(pw, KINDS[SLIDER], one, count=-1) == ERR_INVALID and ul.message(pw) == "phx_world_add_sliders: negative count -1"
    assert ul.raw_add(pw, KINDS[SLIDER], one, null=True) == ERR_INVALID and ul.message(pw) == "phx_world_add_sliders: null array"
    assert ul.raw_add(pw, KINDS[SLIDER], np.zeros(0, dtype=slider_dtype), count=0, null=True) == 0, "an empty call is a true no-op"
    ul.unchanged(pw, before)
    ns = pw.slider_count()
    calls = {"phx_world_remove_sliders": lambda which: pw.remove_sliders(which),
             "phx_world_set_slider_anchors": lambda which: pw.set_slider_anchors(which, np.zeros((len(which), 4), dtype=np.float32)),
             "phx_world_set_slider_limits": lambda which: pw.set_slider_limits(which, np.zeros((len(which), 2), dtype=np.float32)),
             "phx_world_set_slider_motors": lambda which: pw.set_slider_motors(which, np.ones((len(which), 2), dtype=np.float32))}
    for which, tail in (([ns], "slider index %d out of range [0, %d)" % (ns, ns)), ([-1], "slider index -1 out of range [0, %d)" % ns),
                        ([1, 1], "slider 1 appears twice in one call")):
        for name, call in calls.items():
            with pytest.raises(PhxError) as e:
                call(which)
            assert e.value.status == ERR_INVALID and str(e.value).endswith(name + ": " + tail), str(e.value)
            ul.unchanged(pw, before)
    spring = pw.add_sliders([(0, 1, O, O, X, 0.1, 0.1, 2.0, 0.5)])[0]
    before = ul.snapshot_of(pw)
    L = "phx_world_set_slider_limits: slider 0: "
    for which, limits, message in (([0], [1.0, np.nan], L + "a limit is not finite"), ([0], [3.0, 2.0], L + "limits [3, 2] are not lower <= upper"),
                                   ([int(spring)], [1.0, 2.0], L + "a spring (hertz 2) needs lower == upper")):
        with pytest.raises(PhxError) as e:
            pw.set_slider_limits(which, np.array([limits], dtype=np.float32))
        assert e.value.status == ERR_INVALID and str(e.value).endswith(message), str(e.value)
        ul.unchanged(pw, before)
    M = "phx_world_set_slider_motors: slider 0: "
    for motors, message in (([np.inf, 1.0], M + "a motor value is not finite"), ([1.0, np.nan], M + "a motor value is not finite"),
                            ([1.0, -2.0], M + "negative max_force -2")):
        with pytest.raises(PhxError) as e:
            pw.set_slider_motors([0], np.array([motors], dtype=np.float32))
        assert e.value.status == ERR_INVALID and str(e.value).endswith(message), str(e.value)
        ul.unchanged(pw, before)
    with pytest.raises(PhxError) as e:
        pw.set_slider_anchors([0], np.array([[0.0, 0.0, np.nan, 0.0]], dtype=np.float32))
    assert e.value.status == ERR_INVALID and str(e.value).endswith("phx_world_set_slider_anchors: entry 0: value 2 is not finite"), str(e.value)
    ul.unchanged(pw, before)
    idx = np.zeros(1, dtype=np.int32)
    ip = idx.ctypes.data_as(C.c_void_p)
    assert pw.L.phx_world_remove_sliders(pw.h, None, 1) == ERR_INVALID and ul.message(pw) == "phx_world_remove_sliders: null array"
    assert pw.L.phx_world_remove_sliders(pw.h, ip, -1) == ERR_INVALID and ul.message(pw) == "phx_world_remove_sliders: negative count -1"
    assert pw.L.phx_world_set_slider_anchors(pw.h, ip, None, 1) == ERR_INVALID and ul.message(pw) == "phx_world_set_slider_anchors: null array"
    assert pw.L.phx_world_set_slider_limits(pw.h, ip, None, 1) == ERR_INVALID and ul.message(pw) == "phx_world_set_slider_limits: null array"
    assert pw.L.phx_world_set_slider_motors(pw.h, ip, None, 1) == ERR_INVALID and ul.message(pw) == "phx_world_set_slider_motors: null array"
    out = np.zeros(1, dtype=slider_dtype)
    assert pw.L.phx_world_get_sliders(pw.h, out.ctypes.data_as(C.c_void_p), 1) == ERR_CAPACITY
    assert ul.message(pw) == "phx_world_get_sliders: room for 1 sliders, the world has %d" % pw.slider_count()
    pw.remove_sliders([]); pw.set_slider_limits([], np.zeros((0, 2), dtype=np.float32)); pw.set_slider_motors([], np.zeros((0, 2), dtype=np.float32))
    pw.set_slider_anchors([], np.zeros((0, 4), dtype=np.float32))
    ul.unchanged(pw, before)
    # inside a step every call is refused
    pw.PreSolve(DT)
    for call in (lambda: pw.add_sliders(one), lambda: pw.remove_sliders([0]), lambda: pw.set_slider_limits([0], np.zeros((1, 2), dtype=np.float32)),
                 lambda: pw.set_slider_motors([0], np.ones((1, 2), dtype=np.float32)), lambda: pw.set_slider_anchors([0], np.zeros((1, 4), dtype=np.float32))):
        with pytest.raises(PhxError) as e:
            call()
        assert e.value.status == ERR_STATE
    pw.FinishStep(DT, cfg)
    assert pw.slider_count() == ns + 1
