"""Angles on the device (include/phyx_amd.h ANGLES) held to their specification, tests/angle_spec.py, in the lockstep of
tests/unit_lockstep.py; then the schedule's paths, the life cycle by twins, and the refusals.  (What every kind of unit has alike is in
tests/test_units_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import phyx_amd
from phyx_amd import PhxError
from phyx_amd.api import angle_dtype
from angle_corpus import rows_of as _rows_of
import angle_spec
import removal_spec
import unit_lockstep as ul
from unit_lockstep import DT, G, MODES, ERR_INVALID, ERR_CAPACITY, ERR_STATE, lists
from unit_scenes import MIXED, limited_chain as _limited_chain, mixed_world
from unit_spec import ANGLE, KINDS

pytestmark = pytest.mark.gpu


def _step(oracle, pw, ow, cfg, units):
    """-> (the schedule, the angles' prestep records)"""
    sched, work = ul.step(oracle, pw, ow, cfg, units)
    return sched, work[ANGLE]


def _lockstep(oracle, pw, ow, cfg, units, steps):
    """-> (the last schedule, per step the angles' engaged rows)"""
    states = []
    for s in range(steps):
        sched, work = _step(oracle, pw, ow, cfg, units)
        ul.check(pw, ow, units, s)
        states.append([_rows_of(w) for w in work])
    return sched, states


# ---- one body on one world angle ----
@pytest.mark.parametrize("kind", ["lock", "limit", "spring", "motor"])
def test_one_body_on_a_world_angle(oracle, built_lib, kind):
    body = [(0.0, 100.0, 3.0, 1.0, False, 0.4)]
    angle = {"lock": (0, -1, 0.1, 0.1), "limit": (0, -1, -0.5, 0.5), "spring": (0, -1, 0.0, 0.0, 2.0, 0.3),
             "motor": (0, -1, -100.0, 100.0, 0.0, 0.0, 3.0, 2.0e-5)}[kind]      # (weak: still accelerating, its impulse at the clamp, after 60 steps)
    angles = angle_spec.make_angles([angle])
    pw, ow = ul.worlds(ul.scene(body), lists(angles=angles))
    assert pw.angle_count() == 1 and pw.pin_count() == 0 and pw.link_count() == 0
    assert pw.angles().tobytes() == angles.tobytes(), "before the first step the angles wait on the host"
    if kind == "limit":
        pw.set_velocities([0], np.array([[0.0, 0.0, 3.0]], dtype=np.float32))      # theta falls by 0.05 a step: past -0.5 after 18
        ow.bodies()["angular_velocity"][0] = 3.0
    sched, states = _lockstep(oracle, pw, ow, ul.cfg(), lists(angles=angles), 60)
    assert sched["lds_groups"] == 1 and len(sched["class_offsets"]) == 2
    flat = [s[0] for s in states]
    if kind == "limit":
        first = flat.index("L")
        assert first > 10 and set(flat[:first]) == {"idle"} and set(flat[first:]) == {"L"}, "the limit was idle, then engaged"
        assert angles["impulse"][0] >= 0
    elif kind == "motor":
        assert set(flat) == {"M"} and angles["motor_impulse"][0] != 0 and angles["impulse"][0] == 0
    else:
        assert set(flat) == {"L"} and angles["impulse"][0] != 0
    assert pw.pin_schedule_builds() == 1


# ---- among contacts ----
def _door():
    """a static ground, a door (a tall box pinned to the world at its foot, leaning 0.15, limited to +-0.4 against the world) that tips
    over against its stop, and a box that falls on it there -> (body rows, pins, angles)"""
    rows = [(0.0, 0.0, 60.0, 2.0, True), (-0.9, 19.9, 1.0, 6.0, False, 0.15), (-3.5, 36.0, 2.0, 2.0, False)]
    return rows, ul.pins([(1, -1, (0.0, -6.0), (0.0, 14.0))]), angle_spec.make_angles([(1, -1, -0.4, 0.4)])


@pytest.mark.parametrize("mode", list(MODES))
def test_a_limited_door_among_contacts(oracle, built_lib, mode):
    rows, pins, angles = _door()
    pw, ow = ul.worlds(ul.scene(rows), lists(pins=pins, angles=angles))
    touched, rows_seen = False, set()
    for s in range(60):
        _, work = _step(oracle, pw, ow, ul.cfg(MODES[mode]), lists(pins=pins, angles=angles))
        ul.check(pw, ow, lists(pins=pins, angles=angles), s)
        rows_seen.add(_rows_of(work[0]))
        m = pw.manifolds
        touched = touched or bool(((m["body1"] == 1) | (m["body2"] == 1)).any())
    assert pw.pin_schedule_builds() == 1
    assert touched, "the box never hit the door"
    assert rows_seen == {"idle", "L"}, "the door swung freely, then stood against its stop"
    assert np.abs(pins["impulse"]).max() > 0


# ---- the paths ----
@pytest.mark.parametrize("case", ["chain40_cap16", "chain40_pairs_cap16", "chain40", "chain130"])
def test_the_paths(oracle, built_lib, monkeypatch, case):
    """80 units in one component above a cap of 16: the trailing group alone; the same chain beside 20 pairs of a pin and a lock at
    cap 16: LDS groups and the trailing group in one pass; the chain at the default: one LDS group; 260 units in one component, more
    than a workgroup: the HBM path at the default"""
    if case in ("chain40_cap16", "chain40_pairs_cap16"):
        monkeypatch.setenv("PHX_PIN_GROUP_PINS", "16")
    bodies, pins, angles = _limited_chain(130 if case == "chain130" else 40)
    if case == "chain40_pairs_cap16":
        first, pin_rows, angle_rows = len(bodies), [], []
        for k in range(20):
            a = first + 2 * k
            bodies += [(40.0 * k, 300.0, 4.0, 1.5, False, 0.1 * (k % 5)), (40.0 * k + 10.0, 300.0, 4.0, 2.0, False)]
            pin_rows += [(a, a + 1, (5.0, 0.0), (-5.0, 0.0))]
            angle_rows += [(a + 1, a, 0.0, 0.0)]
        pins, angles = np.concatenate([pins, ul.pins(pin_rows)]), np.concatenate([angles, angle_spec.make_angles(angle_rows)])
    pw, ow = ul.worlds(ul.scene(bodies), lists(pins=pins, angles=angles))
    steps = 4 if case == "chain130" else 14
    sched, states = _lockstep(oracle, pw, ow, ul.cfg(), lists(pins=pins, angles=angles), steps)
    lds, groups = sched["lds_groups"], len(sched["group_offsets"]) - 1
    if case == "chain40":
        assert (lds, groups) == (1, 1)
    elif case == "chain40_pairs_cap16":
        assert lds >= 2 and groups == lds + 1, "the pairs in LDS groups, the chain in the trailing group"
    else:
        assert (lds, groups) == (0, 1), "one component that no workgroup takes"
    assert len(sched["order"]) == len(pins) + len(angles)
    assert np.abs(pins["impulse"]).max() > 0
    if case != "chain130":
        assert "L" in {r for s in states for r in s} and np.abs(angles["impulse"]).max() > 0, "no joint of the falling chain reached its limit"


def test_pairs_in_several_groups(oracle, built_lib, monkeypatch):
    """300 pairs, each a pin and a lock or a motor, at cap 64: several LDS groups and no trailing one"""
    monkeypatch.setenv("PHX_PIN_GROUP_PINS", "64")
    bodies, pins, angles = [], [], []
    for k in range(300):
        x, y = 40.0 * (k % 20), 30.0 * (k // 20)
        bodies += [(x, y, 4.0, 1.5, False, 0.1 * (k % 5)), (x + 10.0, y, 3.0 + (k % 3), 2.0, False)]
        pins += [(2 * k, 2 * k + 1, (5.0, 1.0 - 0.1 * (k % 7)), (-5.0, 0.0))]
        angles += [(2 * k + 1, 2 * k, 0.0, 0.0) if k % 2 else (2 * k, 2 * k + 1, -50.0, 50.0, 0.0, 0.0, 1.0 + k % 3, 0.01)]
    pins, angles = ul.pins(pins), angle_spec.make_angles(angles)
    pw, ow = ul.worlds(ul.scene(bodies), lists(pins=pins, angles=angles))
    sched, _ = _lockstep(oracle, pw, ow, ul.cfg(), lists(pins=pins, angles=angles), 4)
    assert sched["lds_groups"] == len(sched["group_offsets"]) - 1 >= 5
    assert np.abs(angles["impulse"]).max() > 0 and np.abs(angles["motor_impulse"]).max() > 0


def test_a_world_with_angles_only(oracle, built_lib):
    bodies = [(30.0 * k, 100.0, 3.0, 1.0, False, 0.2 * k) for k in range(6)]
    angles = angle_spec.make_angles([(1, 0, 0.0, 0.0), (2, 1, -0.1, 0.1), (3, 2, 0.0, 0.0, 1.5, 0.2), (4, 3, -9.0, 9.0, 0.0, 0.0, 2.0, 0.02), (5, -1, 0.0, 0.0)])
    pw, ow = ul.worlds(ul.scene(bodies), lists(angles=angles))
    pw.set_velocities([0], np.array([[0.0, 0.0, 1.5]], dtype=np.float32))
    ow.bodies()["angular_velocity"][0] = 1.5
    sched, states = _lockstep(oracle, pw, ow, ul.cfg(), lists(angles=angles), 12)
    assert pw.pin_count() == 0 and pw.link_count() == 0 and len(sched["order"]) == 5
    assert states[0] == ["L", "L", "L", "M", "L"]


# ---- the life cycle, by twins ----
def _mixed_world():
    return mixed_world("angle")


def test_remove_angles(built_lib):
    pa = _mixed_world()
    for _ in range(8):
        pa.Update(DT, ul.cfg())
    state, pins, links, angles = pa.state(), pa.pins(), pa.links(), pa.angles()
    builds = pa.pin_schedule_builds()
    assert np.abs(angles["impulse"]).max() > 0 and np.abs(angles["motor_impulse"]).max() > 0
    pa.remove_angles([10, 3])
    kept = np.delete(angles, [3, 10])
    assert pa.angles().tobytes() == kept.tobytes(), "the others keep their order"
    ul.run_twins(pa, ul.twin(state, lists(pins=pins, links=links, angles=kept)), 5, "remove_angles")
    assert pa.pin_schedule_builds() == builds + 1


def test_removing_pins_and_links_shifts_the_angle_units(oracle, built_lib):
    bodies, (pins, links, angles, _) = MIXED["angle"]()
    pw, ow = ul.worlds(ul.scene(bodies), lists(pins=pins, links=links, angles=angles))
    cfg = ul.cfg()
    for s in range(4):
        _step(oracle, pw, ow, cfg, lists(pins=pins, links=links, angles=angles))
        ul.check(pw, ow, lists(pins=pins, links=links, angles=angles), s)
    pw.remove_pins([3, 7])
    pw.remove_links([0])
    pins, links = np.delete(pins, [3, 7]), np.delete(links, [0])
    for s in range(4, 8):
        sched, _ = _step(oracle, pw, ow, cfg, lists(pins=pins, links=links, angles=angles))
        ul.check(pw, ow, lists(pins=pins, links=links, angles=angles), s)
    assert len(sched["order"]) == len(pins) + len(links) + len(angles) and pw.pin_schedule_builds() == 2


def test_remove_bodies_through_a_limited_chain(built_lib):
    pa = _mixed_world()
    for _ in range(8):
        pa.Update(DT, ul.cfg())
    state, pins, links, angles = pa.state(), pa.pins(), pa.links(), pa.angles()
    removed = [11, 5]                                       # the middle of the welded pair, and a body in the chain
    filtered = removal_spec.filter(state, removed)
    new = removal_spec.new_index(len(state[0]), removed)
    kept_pins, kept_links, kept_angles = (ul.remapped(u, new) for u in (pins, links, angles))
    assert len(kept_angles) == len(angles) - 4 and len(kept_pins) == len(pins) - 4
    assert pa.remove_bodies(removed).tolist() == new.tolist()
    assert pa.angles().tobytes() == kept_angles.tobytes() and pa.pins().tobytes() == kept_pins.tobytes() and pa.links().tobytes() == kept_links.tobytes()
    pb = ul.twin(filtered[0], lists(pins=kept_pins, links=kept_links, angles=kept_angles))
    ul.same(pa, pb, "right after the removal")
    ul.run_twins(pa, pb, 8, "the removal")


def test_limit_and_motor_edits_keep_the_schedule(oracle, built_lib):
    """on the device: free limits narrowed below the current angle engage at the next step; a motor is switched on, then reversed"""
    bodies = [(0.0, 100.0, 3.0, 1.0, False, 0.3), (50.0, 100.0, 3.0, 1.0, False)]
    angles = angle_spec.make_angles([(0, -1, -1.0, 1.0), (1, -1, -50.0, 50.0)])
    pw, ow = ul.worlds(ul.scene(bodies), lists(angles=angles))
    cfg = ul.cfg()
    for s in range(3):
        _, work = _step(oracle, pw, ow, cfg, lists(angles=angles))
        ul.check(pw, ow, lists(angles=angles), s)
        assert [_rows_of(w) for w in work] == ["idle", "idle"]
    builds = pw.pin_schedule_builds()
    pw.set_angle_limits([0], np.array([[-0.1, 0.1]], dtype=np.float32))
    angles["lower"][0], angles["upper"][0] = -0.1, 0.1
    pw.set_angle_motors([1], np.array([[2.0, 0.01]], dtype=np.float32))
    angles["motor_speed"][1], angles["max_torque"][1] = 2.0, 0.01
    assert pw.angles().tobytes() == angles.tobytes()
    for s in range(3, 6):
        _, work = _step(oracle, pw, ow, cfg, lists(angles=angles))
        ul.check(pw, ow, lists(angles=angles), s)
        assert [_rows_of(w) for w in work] == ["L", "M"]
        pushed = angles["impulse"][0] < 0 if s == 3 else pushed
    assert pushed, "the narrowed limit pushed back at the step after the edit (afterwards the body coasts back with impulse 0)"
    assert angles["motor_impulse"][1] > 0
    pw.set_angle_motors([1, 0], np.array([[-2.0, 0.01], [0.5, 0.002]], dtype=np.float32))
    angles["motor_speed"][1] = -2.0
    angles["motor_speed"][0], angles["max_torque"][0] = 0.5, 0.002
    for s in range(6, 9):
        _, work = _step(oracle, pw, ow, cfg, lists(angles=angles))
        ul.check(pw, ow, lists(angles=angles), s)
        assert [_rows_of(w) for w in work] == ["LM", "M"]
    assert pw.pin_schedule_builds() == builds == 1


def test_edits_before_the_first_step_are_host_staged(built_lib):
    pa, pb = _mixed_world(), _mixed_world()
    angles = pa.angles()
    pa.set_angle_limits([2, 10], np.array([[-0.05, 0.4], [0.1, 0.1]], dtype=np.float32))
    pa.set_angle_motors([11, 0], np.array([[-3.0, 0.1], [1.0, 0.02]], dtype=np.float32))
    angles["lower"][2], angles["upper"][2] = -0.05, 0.4
    angles["lower"][10], angles["upper"][10] = 0.1, 0.1
    angles["motor_speed"][11], angles["max_torque"][11] = -3.0, 0.1
    angles["motor_speed"][0], angles["max_torque"][0] = 1.0, 0.02
    assert pa.angles().tobytes() == angles.tobytes() and pa.pin_schedule_builds() == 0
    pb.remove_angles(list(range(len(angles))))
    pb.add_angles(angles)
    ul.run_twins(pa, pb, 4, "host-staged edits")
    assert pa.pin_schedule_builds() == 1


def test_save_load_and_fork(built_lib):
    cfg = ul.cfg()
    pw = _mixed_world()
    for _ in range(6):
        pw.Update(DT, cfg)
    snap = pw.save()
    saved = (pw.pins().tobytes(), pw.links().tobytes(), pw.angles().tobytes())
    assert np.abs(pw.angles()["impulse"]).max() > 0 and np.abs(pw.angles()["motor_impulse"]).max() > 0
    first = []
    for _ in range(8):
        pw.Update(DT, cfg)
        first.append((pw.bodies.tobytes(), pw.pins().tobytes(), pw.links().tobytes(), pw.angles().tobytes()))
    other = phyx_amd.World(0, gravity=G)
    other.load(snap)
    pw.load(snap)
    assert (pw.pins().tobytes(), pw.links().tobytes(), pw.angles().tobytes()) == saved == (other.pins().tobytes(), other.links().tobytes(), other.angles().tobytes())
    for s in range(8):
        pw.Update(DT, cfg)
        other.Update(DT, cfg)
        assert (pw.bodies.tobytes(), pw.pins().tobytes(), pw.links().tobytes(), pw.angles().tobytes()) == first[s], "the loaded world differs at step %d" % s
        assert (other.bodies.tobytes(), other.pins().tobytes(), other.links().tobytes(), other.angles().tobytes()) == first[s], "the fork differs at step %d" % s


# ---- the refusals ----
GOOD = (0, 1, -0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def _bad(**fields):
    p = np.array([GOOD, GOOD], dtype=angle_dtype)
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
    A = "phx_world_add_angles: angle 1: "
    bad = [(dict(body1=-1), A + "body1 -1 out of range [0, %d)" % n), (dict(body1=n), A + "body1 %d out of range [0, %d)" % (n, n)),
           (dict(body2=n), A + "body2 %d is neither -1 nor in [0, %d)" % (n, n)), (dict(body2=-2), A + "body2 -2 is neither -1 nor in [0, %d)" % n),
           (dict(body1=2, body2=2), A + "both ends on body 2"),
           (dict(lower=np.nan), A + "value 0 is not finite"), (dict(upper=np.inf), A + "value 1 is not finite"), (dict(hertz=np.nan), A + "value 2 is not finite"),
           (dict(damping_ratio=-np.inf), A + "value 3 is not finite"), (dict(motor_speed=np.inf), A + "value 4 is not finite"),
           (dict(max_torque=np.nan), A + "value 5 is not finite"), (dict(impulse=np.nan), A + "value 6 is not finite"),
           (dict(motor_impulse=-np.inf), A + "value 7 is not finite"),
           (dict(hertz=-1.0), A + "negative hertz or damping_ratio"), (dict(damping_ratio=-0.5), A + "negative hertz or damping_ratio"),
           (dict(lower=1.0), A + "limits [1, 0.5] are not lower <= upper"),
           (dict(hertz=2.0), A + "a spring (hertz 2) needs lower == upper"),
           (dict(max_torque=-1.0), A + "negative max_torque -1")]
    for fields, message in bad:
        assert ul.raw_add(pw, KINDS[ANGLE], _bad(**fields)) == ERR_INVALID, fields
        assert ul.message(pw) == message
        ul.unchanged(pw, before)
    assert ul.raw_add(pw, KINDS[ANGLE], _bad(hertz=2.0, lower=0.5)) == 0, "a spring with lower == upper is fine"
    pw.remove_angles([pw.angle_count() - 1, pw.angle_count() - 2])
    before = ul.snapshot_of(pw)
    one = np.array([GOOD], dtype=angle_dtype)
    assert ul.raw_add(pw, KINDS[ANGLE], one, count=-1) == ERR_INVALID and ul.message(pw) == "phx_world_add_angles: negative count -1"
    assert ul.raw_add(pw, KINDS[ANGLE], one, null=True) == ERR_INVALID and ul.message(pw) == "phx_world_add_angles: null array"
    assert ul.raw_add(pw, KINDS[ANGLE], np.zeros(0, dtype=angle_dtype), count=0, null=True) == 0, "an empty call is a true no-op"
    ul.unchanged(pw, before)
    na = pw.angle_count()
    calls = {"phx_world_remove_angles": lambda which: pw.remove_angles(which),
             "phx_world_set_angle_limits": lambda which: pw.set_angle_limits(which, np.zeros((len(which), 2), dtype=np.float32)),
             "phx_world_set_angle_motors": lambda which: pw.set_angle_motors(which, np.ones((len(which), 2), dtype=np.float32))}
    for which, tail in (([na], "angle index %d out of range [0, %d)" % (na, na)), ([-1], "angle index -1 out of range [0, %d)" % na),
                        ([1, 1], "angle 1 appears twice in one call")):
        for name, call in calls.items():
            with pytest.raises(PhxError) as e:
                call(which)
            assert e.value.status == ERR_INVALID and str(e.value).endswith(name + ": " + tail), str(e.value)
            ul.unchanged(pw, before)
    spring = pw.add_angles([(0, 1, 0.1, 0.1, 2.0, 0.5)])[0]
    before = ul.snapshot_of(pw)
    L = "phx_world_set_angle_limits: angle 0: "
    for which, limits, message in (([0], [1.0, np.nan], L + "a limit is not finite"), ([0], [3.0, 2.0], L + "limits [3, 2] are not lower <= upper"),
                                   ([int(spring)], [1.0, 2.0], L + "a spring (hertz 2) needs lower == upper")):
        with pytest.raises(PhxError) as e:
            pw.set_angle_limits(which, np.array([limits], dtype=np.float32))
        assert e.value.status == ERR_INVALID and str(e.value).endswith(message), str(e.value)
        ul.unchanged(pw, before)
    M = "phx_world_set_angle_motors: angle 0: "
    for motors, message in (([np.inf, 1.0], M + "a motor value is not finite"), ([1.0, np.nan], M + "a motor value is not finite"),
                            ([1.0, -2.0], M + "negative max_torque -2")):
        with pytest.raises(PhxError) as e:
            pw.set_angle_motors([0], np.array([motors], dtype=np.float32))
        assert e.value.status == ERR_INVALID and str(e.value).endswith(message), str(e.value)
        ul.unchanged(pw, before)
    idx = np.zeros(1, dtype=np.int32)
    assert pw.L.phx_world_remove_angles(pw.h, None, 1) == ERR_INVALID and ul.message(pw) == "phx_world_remove_angles: null array"
    assert pw.L.phx_world_remove_angles(pw.h, idx.ctypes.data_as(C.c_void_p), -1) == ERR_INVALID and ul.message(pw) == "phx_world_remove_angles: negative count -1"
    assert pw.L.phx_world_set_angle_limits(pw.h, idx.ctypes.data_as(C.c_void_p), None, 1) == ERR_INVALID and ul.message(pw) == "phx_world_set_angle_limits: null array"
    assert pw.L.phx_world_set_angle_motors(pw.h, idx.ctypes.data_as(C.c_void_p), None, 1) == ERR_INVALID and ul.message(pw) == "phx_world_set_angle_motors: null array"
    out = np.zeros(1, dtype=angle_dtype)
    assert pw.L.phx_world_get_angles(pw.h, out.ctypes.data_as(C.c_void_p), 1) == ERR_CAPACITY
    assert ul.message(pw) == "phx_world_get_angles: room for 1 angles, the world has %d" % pw.angle_count()
    pw.remove_angles([]); pw.set_angle_limits([], np.zeros((0, 2), dtype=np.float32)); pw.set_angle_motors([], np.zeros((0, 2), dtype=np.float32))
    ul.unchanged(pw, before)
    # inside a step every call is refused
    pw.PreSolve(DT)
    for call in (lambda: pw.add_angles(one), lambda: pw.remove_angles([0]), lambda: pw.set_angle_limits([0], np.zeros((1, 2), dtype=np.float32)),
                 lambda: pw.set_angle_motors([0], np.ones((1, 2), dtype=np.float32))):
        with pytest.raises(PhxError) as e:
            call()
        assert e.value.status == ERR_STATE
    pw.FinishStep(DT, cfg)
    assert pw.angle_count() == na + 1
