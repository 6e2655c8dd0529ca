"""Angles on the device (include/phyx_amd.h ANGLES) held to their specification, tests/angle_spec.py: the device World and the oracle
World in lockstep, the spec's pass over pins, links and angles applied to the oracle's bodies between its pre_solve and its solve on
the device's own schedule of units, every byte of the state, of the pins, of the links and of the angles compared after every step;
then the schedule's paths, the life cycle by twins, and the refusals.  (The lockstep is that of tests/test_links_gpu.py with the third
list.)"""
import ctypes as C

import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration, PhxError, scenes
from phyx_amd.api import angle_dtype, link_dtype, pin_dtype
from helpers import oracle_world
from spawn_lockstep import compare
import angle_spec
import link_spec
import removal_spec

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
NAMES = ("bodies", "manifolds", "contact points", "joints")
MODES = {"single": phyx_amd.ISLAND_SINGLE, "multiple_sloppy": phyx_amd.ISLAND_MULTIPLE_SLOPPY}
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -4, -5
NO_PINS = np.zeros(0, dtype=pin_dtype)
NO_LINKS = np.zeros(0, dtype=link_dtype)


def _cfg(mode=phyx_amd.ISLAND_MULTIPLE_SLOPPY, iters=15):
    return Configuration(phyx_amd.SOLVE_AVX2, mode, iters, iters)


def _scene(rows):
    """rows (px, py, half_x, half_y, static[, angle]) -> a scenes.py dict"""
    r = np.asarray([row[:4] for row in rows], dtype=np.float32).reshape(-1, 4)
    return {"px": r[:, 0].copy(), "py": r[:, 1].copy(), "angle": np.asarray([row[5] if len(row) > 5 else 0.0 for row in rows], dtype=np.float32),
            "sx": r[:, 2].copy(), "sy": r[:, 3].copy(), "static": np.asarray([bool(row[4]) for row in rows], dtype=bool)}


def _pins(rows):
    p = np.zeros(len(rows), dtype=pin_dtype)
    for k, (a, b, a1, a2) in enumerate(rows):
        p[k] = (a, b, a1, a2, (0.0, 0.0))
    return p


def _worlds(scene, pins, links, angles, gravity=G, with_oracle=True):
    pw = phyx_amd.World(0, gravity=gravity)
    pw.add_scene(scene)
    assert pw.add_pins(pins).tolist() == list(range(len(pins)))
    assert pw.add_links(links).tolist() == list(range(len(links)))
    assert pw.add_angles(angles).tolist() == list(range(len(angles)))
    return pw, (oracle_world(scene, gravity) if with_oracle else None)


def _step(oracle, pw, ow, cfg, pins, links, angles, dt=DT):
    """1. pw.Update  2. ow.pre_solve  3. angle_spec.solve_units on ow.bodies() on the device's own schedule of units  4. the oracle's
    solver on the device's contact schedule  5. ow.integrate_position.  `pins`, `links`, `angles` are the spec's own lists.
    -> (the schedule, the angles' prestep records)"""
    sched = pw.pin_schedule()
    assert sorted(sched["order"].tolist()) == list(range(len(pins) + len(links) + len(angles)))
    pw.Update(dt, cfg)
    ow.pre_solve(dt)
    _, work = angle_spec.solve_units(ow.bodies(), pins, links, angles, sched["order"], dt, pw.pin_iterations)
    order, offs = pw.solver.schedule()
    groups, _ = pw.solver.groups()
    b, cp, j = ow.bodies(), ow.contact_points(), ow.joints()
    assert len(order) == len(j)
    oracle.solver_solve_grouped(b, cp, j, order, offs, groups, cfg.contactIterationsCount, cfg.penetrationIterationsCount, oracle.STAG_COLOUR_SYNC)
    ow.integrate_position(dt)
    return sched, work


def _check(pw, ow, pins, links, angles, s):
    compare(pw, ow, s)
    assert pw.pins().tobytes() == pins.tobytes(), "pins differ at step %d" % s
    assert pw.links().tobytes() == links.tobytes(), "links differ at step %d" % s
    assert pw.angles().tobytes() == angles.tobytes(), "angles differ at step %d" % s


def _rows_of(w):
    return ("L" if w.lrow else "") + ("M" if w.mrow else "") or ("idle" if w.idle else "inactive")


def _lockstep(oracle, pw, ow, cfg, pins, links, angles, steps):
    """-> (the last schedule, per step the angles' engaged rows)"""
    states = []
    for s in range(steps):
        sched, work = _step(oracle, pw, ow, cfg, pins, links, angles)
        _check(pw, ow, pins, links, angles, s)
        states.append([_rows_of(w) for w in work])
    return sched, states


# ---- one body on one world angle ----
@pytest.mark.parametrize("kind", ["lock", "limit", "spring", "motor"])
def test_one_body_on_a_world_angle(oracle, built_lib, kind):
    body = [(0.0, 100.0, 3.0, 1.0, False, 0.4)]
    angle = {"lock": (0, -1, 0.1, 0.1), "limit": (0, -1, -0.5, 0.5), "spring": (0, -1, 0.0, 0.0, 2.0, 0.3),
             "motor": (0, -1, -100.0, 100.0, 0.0, 0.0, 3.0, 2.0e-5)}[kind]      # (weak: still accelerating, its impulse at the clamp, after 60 steps)
    angles = angle_spec.make_angles([angle])
    pw, ow = _worlds(_scene(body), NO_PINS, NO_LINKS, angles)
    assert pw.angle_count() == 1 and pw.pin_count() == 0 and pw.link_count() == 0
    assert pw.angles().tobytes() == angles.tobytes(), "before the first step the angles wait on the host"
    if kind == "limit":
        pw.set_velocities([0], np.array([[0.0, 0.0, 3.0]], dtype=np.float32))      # theta falls by 0.05 a step: past -0.5 after 18
        ow.bodies()["angular_velocity"][0] = 3.0
    sched, states = _lockstep(oracle, pw, ow, _cfg(), NO_PINS, NO_LINKS, angles, 60)
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
    return rows, _pins([(1, -1, (0.0, -6.0), (0.0, 14.0))]), angle_spec.make_angles([(1, -1, -0.4, 0.4)])


@pytest.mark.parametrize("mode", list(MODES))
def test_a_limited_door_among_contacts(oracle, built_lib, mode):
    rows, pins, angles = _door()
    pw, ow = _worlds(_scene(rows), pins, NO_LINKS, angles)
    touched, rows_seen = False, set()
    for s in range(60):
        _, work = _step(oracle, pw, ow, _cfg(MODES[mode]), pins, NO_LINKS, angles)
        _check(pw, ow, pins, NO_LINKS, angles, s)
        rows_seen.add(_rows_of(work[0]))
        m = pw.manifolds
        touched = touched or bool(((m["body1"] == 1) | (m["body2"] == 1)).any())
    assert pw.pin_schedule_builds() == 1
    assert touched, "the box never hit the door"
    assert rows_seen == {"idle", "L"}, "the door swung freely, then stood against its stop"
    assert np.abs(pins["impulse"]).max() > 0


# ---- the paths ----
def _limited_chain(count, top=(0.0, 500.0), spacing=10.0, limit=0.3):
    """`count` boxes level with `top`, pinned end to end from the world point `top`, every joint limited to +-limit
    -> (body rows, pins, angles): 2 count units in one component"""
    h = spacing / 2.0
    bodies = [(top[0] + spacing * (k + 0.5), top[1], 3.0, 1.0, False) for k in range(count)]
    pins = [(0, -1, (-h, 0.0), top)] + [(k, k - 1, (-h, 0.0), (h, 0.0)) for k in range(1, count)]
    angles = [(0, -1, -limit, limit)] + [(k, k - 1, -limit, limit) for k in range(1, count)]
    return bodies, _pins(pins), angle_spec.make_angles(angles)


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
        pins, angles = np.concatenate([pins, _pins(pin_rows)]), np.concatenate([angles, angle_spec.make_angles(angle_rows)])
    pw, ow = _worlds(_scene(bodies), pins, NO_LINKS, angles)
    steps = 4 if case == "chain130" else 14
    sched, states = _lockstep(oracle, pw, ow, _cfg(), pins, NO_LINKS, angles, steps)
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
    pins, angles = _pins(pins), angle_spec.make_angles(angles)
    pw, ow = _worlds(_scene(bodies), pins, NO_LINKS, angles)
    sched, _ = _lockstep(oracle, pw, ow, _cfg(), pins, NO_LINKS, angles, 4)
    assert sched["lds_groups"] == len(sched["group_offsets"]) - 1 >= 5
    assert np.abs(angles["impulse"]).max() > 0 and np.abs(angles["motor_impulse"]).max() > 0


def test_a_world_with_angles_only(oracle, built_lib):
    bodies = [(30.0 * k, 100.0, 3.0, 1.0, False, 0.2 * k) for k in range(6)]
    angles = angle_spec.make_angles([(1, 0, 0.0, 0.0), (2, 1, -0.1, 0.1), (3, 2, 0.0, 0.0, 1.5, 0.2), (4, 3, -9.0, 9.0, 0.0, 0.0, 2.0, 0.02), (5, -1, 0.0, 0.0)])
    pw, ow = _worlds(_scene(bodies), NO_PINS, NO_LINKS, angles)
    pw.set_velocities([0], np.array([[0.0, 0.0, 1.5]], dtype=np.float32))
    ow.bodies()["angular_velocity"][0] = 1.5
    sched, states = _lockstep(oracle, pw, ow, _cfg(), NO_PINS, NO_LINKS, angles, 12)
    assert pw.pin_count() == 0 and pw.link_count() == 0 and len(sched["order"]) == 5
    assert states[0] == ["L", "L", "L", "M", "L"]


# ---- the life cycle, by twins ----
def _same(a, b, what):
    assert a.counts() == b.counts(), "counts differ %s" % what
    for name, x, y in zip(NAMES, a.state(), b.state()):
        assert x.tobytes() == y.tobytes(), "%s differ %s" % (name, what)
    assert a.pins().tobytes() == b.pins().tobytes(), "pins differ %s" % what
    assert a.links().tobytes() == b.links().tobytes(), "links differ %s" % what
    assert a.angles().tobytes() == b.angles().tobytes(), "angles differ %s" % what


def _mixed():
    """a limited chain of 10, a rod across it, a rope from its end, a welded pair (pin + lock) with a motor between the pair and a
    third body -> (body rows, pins, links, angles)"""
    bodies, pins, angles = _limited_chain(10, top=(0.0, 300.0), limit=0.2)
    links = link_spec.make_links([(4, 2, (0.0, 0.0), (0.0, 0.0), 20.0, 20.0), (9, -1, (5.0, 0.0), (100.0, 320.0), 0.0, 12.0)])
    bodies += [(-100.0, 300.0, 4.0, 1.5, False), (-90.0, 300.0, 4.0, 1.5, False), (-80.0, 300.0, 2.0, 2.0, False)]
    pins = np.concatenate([pins, _pins([(10, 11, (5.0, 0.0), (-5.0, 0.0)), (12, 11, (-5.0, 0.0), (5.0, 0.0))])])
    angles = np.concatenate([angles, angle_spec.make_angles([(10, 11, 0.0, 0.0), (12, 11, -50.0, 50.0, 0.0, 0.0, 4.0, 0.05)])])
    return bodies, pins, links, angles


def _mixed_world():
    bodies, pins, links, angles = _mixed()
    pw, _ = _worlds(_scene(bodies), pins, links, angles, with_oracle=False)
    return pw


def _twin(state, pins, links, angles):
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*state)
    pb.add_pins(pins)
    pb.add_links(links)
    pb.add_angles(angles)
    return pb


def _run_twins(pa, pb, steps, what):
    cfg = _cfg()
    for s in range(steps):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "at step %d after %s" % (s, what))


def test_remove_angles(built_lib):
    pa = _mixed_world()
    for _ in range(8):
        pa.Update(DT, _cfg())
    state, pins, links, angles = pa.state(), pa.pins(), pa.links(), pa.angles()
    builds = pa.pin_schedule_builds()
    assert np.abs(angles["impulse"]).max() > 0 and np.abs(angles["motor_impulse"]).max() > 0
    pa.remove_angles([10, 3])
    kept = np.delete(angles, [3, 10])
    assert pa.angles().tobytes() == kept.tobytes(), "the others keep their order"
    _run_twins(pa, _twin(state, pins, links, kept), 5, "remove_angles")
    assert pa.pin_schedule_builds() == builds + 1


def test_removing_pins_and_links_shifts_the_angle_units(oracle, built_lib):
    bodies, pins, links, angles = _mixed()
    pw, ow = _worlds(_scene(bodies), pins, links, angles)
    cfg = _cfg()
    for s in range(4):
        _step(oracle, pw, ow, cfg, pins, links, angles)
        _check(pw, ow, pins, links, angles, s)
    pw.remove_pins([3, 7])
    pw.remove_links([0])
    pins, links = np.delete(pins, [3, 7]), np.delete(links, [0])
    for s in range(4, 8):
        sched, _ = _step(oracle, pw, ow, cfg, pins, links, angles)
        _check(pw, ow, pins, links, angles, s)
    assert len(sched["order"]) == len(pins) + len(links) + len(angles) and pw.pin_schedule_builds() == 2


def test_remove_bodies_through_a_limited_chain(built_lib):
    pa = _mixed_world()
    for _ in range(8):
        pa.Update(DT, _cfg())
    state, pins, links, angles = pa.state(), pa.pins(), pa.links(), pa.angles()
    removed = [11, 5]                                       # the middle of the welded pair, and a body in the chain
    filtered = removal_spec.filter(state, removed)
    new = removal_spec.new_index(len(state[0]), removed)

    def remapped(units):
        keep = np.array([new[p["body1"]] >= 0 and (p["body2"] < 0 or new[p["body2"]] >= 0) for p in units], dtype=bool)
        kept = units[keep].copy()
        kept["body1"] = new[kept["body1"]]
        kept["body2"] = np.where(kept["body2"] < 0, -1, new[np.maximum(kept["body2"], 0)])
        return kept

    kept_pins, kept_links, kept_angles = remapped(pins), remapped(links), remapped(angles)
    assert len(kept_angles) == len(angles) - 4 and len(kept_pins) == len(pins) - 4
    assert pa.remove_bodies(removed).tolist() == new.tolist()
    assert pa.angles().tobytes() == kept_angles.tobytes() and pa.pins().tobytes() == kept_pins.tobytes() and pa.links().tobytes() == kept_links.tobytes()
    pb = _twin(filtered[0], kept_pins, kept_links, kept_angles)
    _same(pa, pb, "right after the removal")
    _run_twins(pa, pb, 8, "the removal")


def test_limit_and_motor_edits_keep_the_schedule(oracle, built_lib):
    """on the device: free limits narrowed below the current angle engage at the next step; a motor is switched on, then reversed"""
    bodies = [(0.0, 100.0, 3.0, 1.0, False, 0.3), (50.0, 100.0, 3.0, 1.0, False)]
    angles = angle_spec.make_angles([(0, -1, -1.0, 1.0), (1, -1, -50.0, 50.0)])
    pw, ow = _worlds(_scene(bodies), NO_PINS, NO_LINKS, angles)
    cfg = _cfg()
    for s in range(3):
        _, work = _step(oracle, pw, ow, cfg, NO_PINS, NO_LINKS, angles)
        _check(pw, ow, NO_PINS, NO_LINKS, angles, s)
        assert [_rows_of(w) for w in work] == ["idle", "idle"]
    builds = pw.pin_schedule_builds()
    pw.set_angle_limits([0], np.array([[-0.1, 0.1]], dtype=np.float32))
    angles["lower"][0], angles["upper"][0] = -0.1, 0.1
    pw.set_angle_motors([1], np.array([[2.0, 0.01]], dtype=np.float32))
    angles["motor_speed"][1], angles["max_torque"][1] = 2.0, 0.01
    assert pw.angles().tobytes() == angles.tobytes()
    for s in range(3, 6):
        _, work = _step(oracle, pw, ow, cfg, NO_PINS, NO_LINKS, angles)
        _check(pw, ow, NO_PINS, NO_LINKS, angles, s)
        assert [_rows_of(w) for w in work] == ["L", "M"]
        pushed = angles["impulse"][0] < 0 if s == 3 else pushed
    assert pushed, "the narrowed limit pushed back at the step after the edit (afterwards the body coasts back with impulse 0)"
    assert angles["motor_impulse"][1] > 0
    pw.set_angle_motors([1, 0], np.array([[-2.0, 0.01], [0.5, 0.002]], dtype=np.float32))
    angles["motor_speed"][1] = -2.0
    angles["motor_speed"][0], angles["max_torque"][0] = 0.5, 0.002
    for s in range(6, 9):
        _, work = _step(oracle, pw, ow, cfg, NO_PINS, NO_LINKS, angles)
        _check(pw, ow, NO_PINS, NO_LINKS, angles, s)
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
    _run_twins(pa, pb, 4, "host-staged edits")
    assert pa.pin_schedule_builds() == 1


def test_save_load_and_fork(built_lib):
    cfg = _cfg()
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


def test_a_snapshot_with_angles_has_no_blob(built_lib):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scenes.stack(2, 3))
    pw.add_angles([(1, -1, -0.5, 0.5)])
    snap = pw.save()
    with pytest.raises(PhxError) as e:
        snap.to_bytes()
    assert e.value.status == ERR_STATE and "the snapshot holds 1 angles, which the blob (layout version 1) does not carry" in str(e.value)
    n = C.c_size_t(0)
    assert pw.L.phx_snapshot_blob_bytes(snap.h, C.byref(n)) == ERR_STATE
    assert pw.L.phx_last_error().decode() == "phx_snapshot_blob_bytes: the snapshot holds 1 angles, which the blob (layout version 1) does not carry"
    pw.remove_angles([0])
    assert len(pw.save().to_bytes()) > 0


def test_set_state_leaves_no_angle(built_lib):
    pw = _mixed_world()
    pw.Update(DT, _cfg())
    pw.set_state(*pw.state())
    assert pw.angle_count() == 0 and len(pw.angles()) == 0 and pw.pin_count() == 0 and pw.link_count() == 0
    pw.Update(DT, _cfg())


def test_a_world_that_lost_its_angles_is_a_world_without(built_lib):
    cfg = _cfg()
    sc = scenes.stack(3, 6)
    pa, pb = phyx_amd.World(0, gravity=G), phyx_amd.World(0, gravity=G)
    pa.add_scene(sc); pb.add_scene(sc)
    pa.add_angles([(1, 2, 0.0, 0.0), (3, -1, -0.2, 0.2, 0.0, 0.0, 1.0, 5.0)])
    pa.remove_angles([0, 1])
    assert pa.angle_count() == 0
    for s in range(10):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        for name, x, y in zip(NAMES, pa.state(), pb.state()):
            assert x.tobytes() == y.tobytes(), "%s differ at step %d" % (name, s)
    assert pa.pin_schedule_builds() == 0, "no units: no schedule, no pass"
    assert pa.save().to_bytes() == pb.save().to_bytes(), "a snapshot without angles is what it was"


# ---- the refusals ----
def _unchanged(pw, before):
    bodies, pins, links, angles, builds = before
    assert pw.bodies.tobytes() == bodies and pw.pins().tobytes() == pins and pw.links().tobytes() == links and pw.angles().tobytes() == angles
    assert pw.pin_schedule_builds() == builds


def _snapshot_of(pw):
    return (pw.bodies.tobytes(), pw.pins().tobytes(), pw.links().tobytes(), pw.angles().tobytes(), pw.pin_schedule_builds())


def _raw_add(pw, angles, count=None, null=False):
    p = np.ascontiguousarray(angles, dtype=angle_dtype)
    return pw.L.phx_world_add_angles(pw.h, None if null else p.ctypes.data_as(C.c_void_p), len(p) if count is None else count, None)


def _message(pw):
    return pw.L.phx_last_error().decode()


GOOD = (0, 1, -0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def _bad(**fields):
    p = np.array([GOOD, GOOD], dtype=angle_dtype)
    for f, v in fields.items():
        p[f][1] = v
    return p


@pytest.mark.parametrize("staged", ["host", "device"])
def test_rejections_leave_the_world_unchanged(built_lib, staged):
    cfg = _cfg()
    pw = _mixed_world()
    if staged == "device":
        pw.Update(DT, cfg)
    n = pw.counts()[0]
    before = _snapshot_of(pw)
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
        assert _raw_add(pw, _bad(**fields)) == ERR_INVALID, fields
        assert _message(pw) == message
        _unchanged(pw, before)
    assert _raw_add(pw, _bad(hertz=2.0, lower=0.5)) == 0, "a spring with lower == upper is fine"
    pw.remove_angles([pw.angle_count() - 1, pw.angle_count() - 2])
    before = _snapshot_of(pw)
    one = np.array([GOOD], dtype=angle_dtype)
    assert _raw_add(pw, one, count=-1) == ERR_INVALID and _message(pw) == "phx_world_add_angles: negative count -1"
    assert _raw_add(pw, one, null=True) == ERR_INVALID and _message(pw) == "phx_world_add_angles: null array"
    assert _raw_add(pw, np.zeros(0, dtype=angle_dtype), count=0, null=True) == 0, "an empty call is a true no-op"
    _unchanged(pw, before)
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
            _unchanged(pw, before)
    spring = pw.add_angles([(0, 1, 0.1, 0.1, 2.0, 0.5)])[0]
    before = _snapshot_of(pw)
    L = "phx_world_set_angle_limits: angle 0: "
    for which, limits, message in (([0], [1.0, np.nan], L + "a limit is not finite"), ([0], [3.0, 2.0], L + "limits [3, 2] are not lower <= upper"),
                                   ([int(spring)], [1.0, 2.0], L + "a spring (hertz 2) needs lower == upper")):
        with pytest.raises(PhxError) as e:
            pw.set_angle_limits(which, np.array([limits], dtype=np.float32))
        assert e.value.status == ERR_INVALID and str(e.value).endswith(message), str(e.value)
        _unchanged(pw, before)
    M = "phx_world_set_angle_motors: angle 0: "
    for motors, message in (([np.inf, 1.0], M + "a motor value is not finite"), ([1.0, np.nan], M + "a motor value is not finite"),
                            ([1.0, -2.0], M + "negative max_torque -2")):
        with pytest.raises(PhxError) as e:
            pw.set_angle_motors([0], np.array([motors], dtype=np.float32))
        assert e.value.status == ERR_INVALID and str(e.value).endswith(message), str(e.value)
        _unchanged(pw, before)
    idx = np.zeros(1, dtype=np.int32)
    assert pw.L.phx_world_remove_angles(pw.h, None, 1) == ERR_INVALID and _message(pw) == "phx_world_remove_angles: null array"
    assert pw.L.phx_world_remove_angles(pw.h, idx.ctypes.data_as(C.c_void_p), -1) == ERR_INVALID and _message(pw) == "phx_world_remove_angles: negative count -1"
    assert pw.L.phx_world_set_angle_limits(pw.h, idx.ctypes.data_as(C.c_void_p), None, 1) == ERR_INVALID and _message(pw) == "phx_world_set_angle_limits: null array"
    assert pw.L.phx_world_set_angle_motors(pw.h, idx.ctypes.data_as(C.c_void_p), None, 1) == ERR_INVALID and _message(pw) == "phx_world_set_angle_motors: null array"
    out = np.zeros(1, dtype=angle_dtype)
    assert pw.L.phx_world_get_angles(pw.h, out.ctypes.data_as(C.c_void_p), 1) == ERR_CAPACITY
    assert _message(pw) == "phx_world_get_angles: room for 1 angles, the world has %d" % pw.angle_count()
    pw.remove_angles([]); pw.set_angle_limits([], np.zeros((0, 2), dtype=np.float32)); pw.set_angle_motors([], np.zeros((0, 2), dtype=np.float32))
    _unchanged(pw, before)
    # inside a step every call is refused
    pw.PreSolve(DT)
    for call in (lambda: pw.add_angles(one), lambda: pw.remove_angles([0]), lambda: pw.set_angle_limits([0], np.zeros((1, 2), dtype=np.float32)),
                 lambda: pw.set_angle_motors([0], np.ones((1, 2), dtype=np.float32))):
        with pytest.raises(PhxError) as e:
            call()
        assert e.value.status == ERR_STATE
    pw.FinishStep(DT, cfg)
    assert pw.angle_count() == na + 1


def test_the_schedule_call_needs_room_for_all_three_kinds(built_lib):
    pw = _mixed_world()
    n = pw.pin_count() + pw.link_count() + pw.angle_count()
    nc, ng, lg = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert pw.L.phx_world_get_pin_schedule(pw.h, None, 0, None, 0, C.byref(nc), None, 0, C.byref(ng), C.byref(lg)) == 0
    order = np.zeros(n, dtype=np.int32)
    coff, goff = np.zeros(nc.value + 1, dtype=np.int32), np.zeros(ng.value + 1, dtype=np.int32)
    args = (coff.ctypes.data_as(C.c_void_p), len(coff), C.byref(nc), goff.ctypes.data_as(C.c_void_p), len(goff), C.byref(ng), C.byref(lg))
    assert pw.L.phx_world_get_pin_schedule(pw.h, order.ctypes.data_as(C.c_void_p), n - 1, *args) == ERR_CAPACITY
    assert _message(pw) == "phx_world_get_pin_schedule: arrays too small"
    assert pw.L.phx_world_get_pin_schedule(pw.h, order.ctypes.data_as(C.c_void_p), n, *args) == 0
    assert sorted(order.tolist()) == list(range(n))


def test_sharded_worlds_carry_no_angles(built_lib):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scenes.stack(2, 3))
    stop = angle_spec.make_angles([(1, -1, -0.5, 0.5)])
    pw.add_angles(stop)
    with pytest.raises(PhxError) as e:
        pw.set_shard(0, 2)
    assert e.value.status == ERR_STATE and str(e.value).endswith("phx_world_set_shard: the world holds angles, which a sharded world does not carry")
    n = pw.counts()[0]
    with pytest.raises(PhxError) as e:
        pw.reslab(np.arange(n, dtype=np.int64), n, (-1e9, 1e9))
    assert e.value.status == ERR_STATE and str(e.value).endswith("phx_world_reslab: the world holds angles, which a sharded world does not carry")
    pw.set_shard(0, 1)
    sharded = phyx_amd.World(0, gravity=G)
    sharded.add_scene(scenes.stack(2, 3))
    sharded.set_shard(0, 2)
    with pytest.raises(PhxError) as e:
        sharded.add_angles(stop)
    assert e.value.status == ERR_STATE and str(e.value).endswith("phx_world_add_angles: a sharded world carries no angles") and sharded.angle_count() == 0


def test_set_comm_refuses_a_world_with_angles(built_lib):
    """as tests/test_links_gpu.py: in a child process, so that RCCL's bootstrap cannot hang the suite's"""
    import os
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "angles_comm_worker.py")
    env = dict(os.environ, PHX_COMM_TIMEOUT_S="60")
    for attempt in range(2):
        p = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=300)
        if "NO COMMUNICATOR" not in p.stdout:
            break
    if "NO COMMUNICATOR" in p.stdout:
        pytest.skip("no RCCL communicator on this box: " + p.stdout[-300:])
    assert p.returncode == 0 and "angles comm worker ok" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]
