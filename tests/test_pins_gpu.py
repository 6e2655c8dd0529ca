"""Pins on the device (include/phyx_amd.h PINS) held to their specification, tests/pin_spec.py, in the lockstep of
tests/unit_lockstep.py; then the schedule's paths, the life cycle by twins, and the refusals.  (What every kind of unit has alike is in
tests/test_units_gpu.py.)"""
import numpy as np
import pytest

import phyx_amd
from phyx_amd import PhxError, scenes
from phyx_amd.api import pin_dtype
import removal_spec
import unit_lockstep as ul
from unit_lockstep import DT, G, MODES, ERR_INVALID, ERR_STATE, lists
from unit_scenes import chain as _chain, mixed_world
from unit_spec import KINDS, PIN

pytestmark = pytest.mark.gpu

ITERS = 8


def _join(base, rows):
    extra = ul.scene(rows)
    return {k: np.concatenate([base[k], extra[k]]) for k in ("px", "py", "angle", "sx", "sy", "static")}


def _worlds(scene, pins):
    return ul.worlds(scene, lists(pins=pins))


def _lockstep(oracle, pw, ow, cfg, pins, steps, watch=slice(None)):
    """-> (the last schedule, the lowest pos.y the bodies `watch` reached)"""
    lowest = np.inf
    for s in range(steps):
        sched, _ = ul.step(oracle, pw, ow, cfg, lists(pins=pins))
        ul.check(pw, ow, lists(pins=pins), s)
        lowest = min(lowest, float(ow.bodies()["pos"]["y"][watch].min()))
    return sched, lowest


def test_one_body_on_a_world_pin(oracle, built_lib):
    bodies, rows = _chain(0, 1, (0.0, 100.0))
    pins = ul.pins(rows)
    pw, ow = _worlds(ul.scene(bodies), pins)
    assert pw.pin_iterations == ITERS and pw.pin_count() == 1
    assert pw.pins().tobytes() == pins.tobytes(), "before the first step the pins wait on the host"
    sched, lowest = _lockstep(oracle, pw, ow, ul.cfg(), pins, 60)
    assert sched["lds_groups"] == 1 and len(sched["class_offsets"]) == 2
    assert np.abs(pins["impulse"]).max() > 0 and lowest < 96.0, "the pendulum never swung"


def test_chains_and_pairs(oracle, built_lib):
    """a pair of dynamic bodies, a 3-chain (two classes) and a 12-chain hung from a static body"""
    bodies = [(-100.0, 200.0, 4.0, 1.5, False), (-90.0, 200.0, 6.0, 2.0, False)]
    rows = [(0, 1, (5.0, 1.0), (-5.0, 0.0))]
    b3, p3 = _chain(2, 3, (0.0, 200.0))
    bodies += b3; rows += p3
    bodies += [(200.0, 200.0, 5.0, 5.0, True)]
    b12, p12 = _chain(6, 12, (205.0, 200.0), hang_from=5, hang_anchor=(5.0, 0.0))
    bodies += b12; rows += p12
    pins = ul.pins(rows)
    pw, ow = _worlds(ul.scene(bodies), pins)
    sched, lowest = _lockstep(oracle, pw, ow, ul.cfg(), pins, 40, watch=slice(6, None))
    assert sched["lds_groups"] == 1 and len(sched["group_offsets"]) == 2
    assert len(sched["class_offsets"]) - 1 == 2, "chains need two classes"
    b = pw.bodies
    assert (b["pos"]["x"][5], b["pos"]["y"][5]) == (200.0, 200.0), "the static body moved"
    assert lowest < 190.0, "the chain never swung"


@pytest.mark.parametrize("mode", list(MODES))
def test_pins_among_contacts(oracle, built_lib, mode):
    """scenes.stack(4, 10), an 8-chain dropped onto it, two neighbouring boxes of a column pinned to each other; the world pin's
    anchor moves at step 20"""
    base = scenes.stack(4, 10)
    n = len(base["px"])
    chain_bodies, rows = _chain(n, 8, (-45.0, 135.0))
    rows += [(4, 5, (0.0, 5.0), (0.0, -5.0))]
    pins = ul.pins(rows)
    pw, ow = _worlds(_join(base, chain_bodies), pins)

    def at(s):
        if s == 20:
            moved = np.array([[-5.0, 0.0, -40.0, 138.0]], dtype=np.float32)
            pw.set_pin_anchors([0], moved)
            pins["anchor1"][0], pins["anchor2"][0] = moved[0, :2], moved[0, 2:]

    builds = None
    for s in range(40):
        at(s)
        ul.step(oracle, pw, ow, ul.cfg(MODES[mode]), lists(pins=pins))
        ul.check(pw, ow, lists(pins=pins), s)
        builds = builds or pw.pin_schedule_builds()
    assert pw.pin_schedule_builds() == builds == 1, "an anchor edit keeps the schedule"
    m = pw.manifolds
    assert ((m["body1"] >= n) | (m["body2"] >= n)).any(), "the chain never touched the stack"


def _pairs(count):
    bodies, rows = [], []
    for k in range(count):
        x, y = 40.0 * (k % 20), 30.0 * (k // 20)
        bodies += [(x, y, 4.0, 1.5, False), (x + 10.0, y, 3.0 + (k % 3), 2.0, False)]
        rows += [(2 * k, 2 * k + 1, (5.0, 1.0 - 0.1 * (k % 7)), (-5.0, 0.0))]
    return bodies, rows


@pytest.mark.parametrize("case", ["pairs300_cap64", "chain40_cap16", "chain40", "pairs5_chain40_cap16"])
def test_the_paths(oracle, built_lib, monkeypatch, case):
    """several LDS groups; the trailing group out of HBM; one workgroup; an LDS group AND an active trailing group (whose slots then
    start behind the LDS group's: the absolute slot offsets and the work array's base)"""
    if case == "pairs300_cap64":
        monkeypatch.setenv("PHX_PIN_GROUP_PINS", "64")
        bodies, rows = _pairs(300)
        steps, lds, groups = 6, 5, 5
    elif case == "pairs5_chain40_cap16":
        monkeypatch.setenv("PHX_PIN_GROUP_PINS", "16")
        bodies, rows = _pairs(5)
        chain_bodies, chain_rows = _chain(10, 40, (0.0, 500.0))
        bodies, rows = bodies + chain_bodies, rows + chain_rows
        steps, lds, groups = 12, 1, 2
    else:
        if case == "chain40_cap16":
            monkeypatch.setenv("PHX_PIN_GROUP_PINS", "16")
        bodies, rows = _chain(0, 40, (0.0, 500.0))
        steps = 12
        lds, groups = (0, 1) if case == "chain40_cap16" else (1, 1)
    pins = ul.pins(rows)
    pw, ow = _worlds(ul.scene(bodies), pins)
    sched, _ = _lockstep(oracle, pw, ow, ul.cfg(), pins, steps)
    assert sched["lds_groups"] == lds and len(sched["group_offsets"]) - 1 == groups
    assert np.abs(pins["impulse"]).max() > 0
    if case == "pairs5_chain40_cap16":
        assert sched["group_offsets"].tolist() == [0, 5, 45], "the pairs in one LDS group, the chain behind them in the trailing group"
        assert np.abs(pins["impulse"][:5]).max() > 0 and np.abs(pins["impulse"][5:]).max() > 0, "both groups are active"


@pytest.mark.parametrize("value", ["0", "257", "x", ""])
def test_group_pins_knob_refuses_other_values(built_lib, monkeypatch, value):
    monkeypatch.setenv("PHX_PIN_GROUP_PINS", value)
    with pytest.raises(PhxError) as e:
        phyx_amd.World(0)
    assert e.value.status == ERR_INVALID


# ---- the life cycle, by twins ----
def _chain_world(links=12, extra_pair=True):
    return mixed_world("pin", links=links, extra_pair=extra_pair)


def test_remove_bodies_through_a_chain(built_lib):
    cfg = ul.cfg()
    pa = _chain_world()
    for _ in range(10):
        pa.Update(DT, cfg)
    state, pins = pa.state(), pa.pins()
    removed = [5]
    filtered = removal_spec.filter(state, removed)
    new = removal_spec.new_index(len(state[0]), removed)
    kept = ul.remapped(pins, new)
    assert len(kept) == len(pins) - 2
    remap = pa.remove_bodies(removed)
    assert remap.tolist() == new.tolist()
    assert pa.pins().tobytes() == kept.tobytes()
    pb = ul.twin(filtered[0], lists(pins=kept))
    ul.same(pa, pb, "right after the removal")
    ul.run_twins(pa, pb, 10, "the removal")


def test_remove_pins(built_lib):
    cfg = ul.cfg()
    pa = _chain_world()
    for _ in range(5):
        pa.Update(DT, cfg)
    state, pins = pa.state(), pa.pins()
    builds = pa.pin_schedule_builds()
    pa.remove_pins([12, 3])
    kept = np.delete(pins, [3, 12])
    assert pa.pins().tobytes() == kept.tobytes(), "the others keep their order"
    ul.run_twins(pa, ul.twin(state, lists(pins=kept)), 5, "remove_pins")
    assert pa.pin_schedule_builds() == builds + 1


def test_what_rebuilds_the_schedule(built_lib):
    cfg = ul.cfg()
    pw = _chain_world()
    pw.Update(DT, cfg)
    builds = pw.pin_schedule_builds()
    assert builds == 1
    pw.set_pin_anchors([0], np.array([[-5.0, 0.0, 2.0, 301.0]], dtype=np.float32))
    pw.add_bodies(np.array([[500.0, 500.0, 0.0, 2.0, 2.0]], dtype=np.float32))
    pw.set_velocities([1], np.array([[1.0, 0.0, 0.0]], dtype=np.float32))
    pw.Update(DT, cfg)
    assert pw.pin_schedule_builds() == builds, "anchor edits, spawns and the other edits keep the schedule"
    assert pw.pins()["anchor2"][0].tolist() == [2.0, 301.0]
    b = pw.bodies
    pw.set_inverse_masses([3], np.array([[b["inv_mass"][3], b["inv_inertia"][3]]], dtype=np.float32))
    pw.Update(DT, cfg)
    assert pw.pin_schedule_builds() == builds + 1, "set_inverse_masses rebuilds it"


def test_a_pin_whose_bodies_became_static(built_lib):
    cfg = ul.cfg()
    pw = _chain_world(links=3)
    for _ in range(5):
        pw.Update(DT, cfg)
    assert np.abs(pw.pins()["impulse"][3]).max() > 0
    pw.set_velocities([3, 4], np.zeros((2, 3), dtype=np.float32))
    pw.set_inverse_masses([3, 4], np.zeros((2, 2), dtype=np.float32))
    before = pw.bodies[[3, 4]]
    for _ in range(3):
        pw.Update(DT, cfg)
    after = pw.bodies[[3, 4]]
    assert after["pos"].tobytes() == before["pos"].tobytes() and after["velocity"].tobytes() == before["velocity"].tobytes(), "static bodies moved"
    pins = pw.pins()
    assert pins["impulse"][3].tolist() == [0.0, 0.0], "an inactive pin reads impulse 0"
    assert np.abs(pins["impulse"][:3]).max() > 0


def test_save_load_and_fork(built_lib):
    cfg = ul.cfg()
    pw = _chain_world()
    pw.pin_iterations = 6
    for _ in range(5):
        pw.Update(DT, cfg)
    snap = pw.save()
    saved_pins = pw.pins()
    first = []
    for _ in range(10):
        pw.Update(DT, cfg)
        first.append((pw.bodies.tobytes(), pw.pins().tobytes()))
    other = phyx_amd.World(0, gravity=G)
    other.pin_iterations = 6
    other.load(snap)
    pw.load(snap)
    assert pw.pins().tobytes() == saved_pins.tobytes() == other.pins().tobytes()
    for s in range(10):
        pw.Update(DT, cfg)
        other.Update(DT, cfg)
        assert (pw.bodies.tobytes(), pw.pins().tobytes()) == first[s], "the loaded world differs at step %d" % s
        assert (other.bodies.tobytes(), other.pins().tobytes()) == first[s], "the fork differs at step %d" % s
    with pytest.raises(PhxError) as e:
        snap.to_bytes()
    assert e.value.status == ERR_STATE and "pins" in str(e.value)


# ---- the refusals ----
@pytest.mark.parametrize("staged", ["host", "device"])
def test_rejections_leave_the_world_unchanged(built_lib, staged):
    import ctypes as C
    cfg = ul.cfg()
    pw = _chain_world(links=4)
    if staged == "device":
        pw.Update(DT, cfg)
    n = pw.counts()[0]
    before = ul.snapshot_of(pw)
    good = (0, 1, (1.0, 0.0), (0.0, 1.0), (0.0, 0.0))
    bad = [(-1, 1), (n, 1), (0, n), (0, -2), (2, 2)]
    for b1, b2 in bad:
        p = np.array([good, (b1, b2, (0.0, 0.0), (0.0, 0.0), (0.0, 0.0))], dtype=pin_dtype)
        assert ul.raw_add(pw, KINDS[PIN], p) == ERR_INVALID, (b1, b2)
        ul.unchanged(pw, before)
    for field, value in (("anchor1", np.nan), ("anchor2", np.inf), ("impulse", -np.inf)):
        p = np.array([good, good], dtype=pin_dtype)
        p[field][1][1] = value
        assert ul.raw_add(pw, KINDS[PIN], p) == ERR_INVALID, field
        ul.unchanged(pw, before)
    assert ul.raw_add(pw, KINDS[PIN], np.array([good], dtype=pin_dtype), count=-1) == ERR_INVALID
    assert ul.raw_add(pw, KINDS[PIN], np.array([good], dtype=pin_dtype), null=True) == ERR_INVALID
    assert ul.raw_add(pw, KINDS[PIN], np.zeros(0, dtype=pin_dtype), count=0, null=True) == 0, "an empty call is a true no-op"
    ul.unchanged(pw, before)
    np_ = pw.pin_count()
    for which in ([np_], [-1], [1, 1]):
        with pytest.raises(PhxError) as e:
            pw.remove_pins(which)
        assert e.value.status == ERR_INVALID
        with pytest.raises(PhxError) as e:
            pw.set_pin_anchors(which, np.zeros((len(which), 4), dtype=np.float32))
        assert e.value.status == ERR_INVALID
        ul.unchanged(pw, before)
    with pytest.raises(PhxError) as e:
        pw.set_pin_anchors([0], np.array([[0.0, np.nan, 0.0, 0.0]], dtype=np.float32))
    assert e.value.status == ERR_INVALID
    idx = np.zeros(1, dtype=np.int32)
    assert pw.L.phx_world_remove_pins(pw.h, None, 1) == ERR_INVALID
    assert pw.L.phx_world_remove_pins(pw.h, idx.ctypes.data_as(C.c_void_p), -1) == ERR_INVALID
    assert pw.L.phx_world_set_pin_anchors(pw.h, idx.ctypes.data_as(C.c_void_p), None, 1) == ERR_INVALID
    pw.remove_pins([]); pw.set_pin_anchors([], np.zeros((0, 4), dtype=np.float32))
    ul.unchanged(pw, before)
    for bad_n in (0, 65, -3):
        with pytest.raises(PhxError) as e:
            pw.pin_iterations = bad_n
        assert e.value.status == ERR_INVALID and pw.pin_iterations == ITERS
    # inside a step every call is refused
    pw.PreSolve(DT)
    for call in (lambda: pw.add_pins(np.array([good], dtype=pin_dtype)), lambda: pw.remove_pins([0]),
                 lambda: pw.set_pin_anchors([0], np.zeros((1, 4), dtype=np.float32)), lambda: setattr(pw, "pin_iterations", 4), pw.pin_schedule):
        with pytest.raises(PhxError) as e:
            call()
        assert e.value.status == ERR_STATE
    pw.FinishStep(DT, cfg)
    assert pw.pin_count() == np_ and pw.pin_iterations == ITERS
