"""Sleeping on the device (include/phyx_amd.h SLEEPING) against its definition (tests/sleep_spec.py) by twins (tests/sleep_lockstep.py):
a world that sleeps is, byte for byte, a world that does not on which the spec's decisions are applied as edits between the steps."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import phyx_amd
from phyx_amd import PhxError, scenes
from unit_lockstep import DT, ERR_INVALID, ERR_STATE, G, MODES, cfg, pins as pin_rows, lists, scene as rows_scene
from sleep_lockstep import Twins
import sleep_oracle
import sleep_spec

pytestmark = pytest.mark.gpu

GENEROUS = (20.0, 5.0, 3 * DT)      # tolerances far above what a resting or a slowly falling box has: calm from the first step


# ---- 1. lockstep twins on tilted(12): the pile settles, sleeps, a dropped box wakes the component it hits -------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_twins_on_the_tilted_pile(mode):
    t = Twins(scenes.tilted(12), sleep_oracle.PARAMS, MODES[mode])
    box = np.array([sleep_oracle.BOX], dtype=np.float32)
    for s in range(520):
        if s == sleep_oracle.BOX_STEP:
            assert t.a.add_bodies(box).tolist() == t.b.add_bodies(box).tolist() == [13]
            t.state = sleep_spec.grown(t.state, 14)
            t.same("after the spawn")
        t.step(s)
    assert max(len(x) for x in t.slept) > 1, "no component of more than one body ever slept"
    assert any(t.woken), "nothing ever woke"
    assert any(0 < len(x) < 12 for x in t.woken[sleep_oracle.BOX_STEP:])   # the box woke a part of the pile, not all of it
    asleep, slept, woken = t.a.sleep_counts()
    assert (slept, woken) == (sum(map(len, t.slept)), sum(map(len, t.woken))) and asleep == slept - woken


# ---- 2. labels at size: one component of 1200 bodies across compress windows and workgroups, beside 300 bodies that stay awake -----
def wall_and_loose(loose=300):
    sc = scenes.wall(40, 30)
    first = len(sc["px"])
    extra = dict(px=500.0 + 12.0 * np.arange(loose), py=np.full(loose, 500.0), angle=np.zeros(loose), sx=np.full(loose, 5.0), sy=np.full(loose, 5.0),
                 static=np.zeros(loose, dtype=bool))
    return {k: np.concatenate([sc[k], np.asarray(extra[k], dtype=sc[k].dtype)]) for k in sc}, first


def test_a_component_larger_than_a_compress_window_sleeps_as_one():
    # (checked on the CPU with the spec and OracleWorld: the wall's boxes fall 0.14 onto each other at <= 10 units/s, far below the
    #  tolerance; the 1200 are one component at step 2 and sleep there; the loose bodies move at 50 and never do)
    sc, first = wall_and_loose()
    loose = np.arange(first, len(sc["px"]))
    fast = np.tile(np.array([50.0, 0.0, 0.0], dtype=np.float32), (len(loose), 1))
    t = Twins(sc, GENEROUS, prepare=lambda w: w.set_velocities(loose, fast))
    for s in range(8):
        t.step(s)
    assert max(len(x) for x in t.slept) > 1024, "no component of more than 1024 bodies slept as one"
    assert not t.state["asleep"][loose].any() and t.state["asleep"][1:first].all()
    assert not any(t.woken)


# ---- 3. units: a hanging chain of pins sleeps as one component and an edit of its top pin wakes it ---------------------------------
def hanging_chain(links=6):
    rows = [(0.0, 300.0 - 10.0 * (k + 0.5), 1.0, 3.0, False) for k in range(links)]
    pins = [(0, -1, (0.0, 5.0), (0.0, 300.0))] + [(k, k - 1, (0.0, 5.0), (0.0, -5.0)) for k in range(1, links)]
    return rows_scene(rows), lists(pins=pin_rows(pins))


def test_a_chain_of_pins_sleeps_as_one_and_its_top_pin_wakes_it():
    # (unit_spec.step_free on the CPU: the chain's rest speed is 7e-3 at step 20 and 1e-6 from step 80 on, below the tilted pile's
    #  tolerances 0.5 / 0.05, which are used as they are)
    sc, units = hanging_chain()
    t = Twins(sc, sleep_oracle.PARAMS, lists=units)
    for s in range(90):
        t.step(s)
        if t.asleep():
            break
    assert t.asleep() == list(range(6)) and t.slept[-1] == list(range(6)), "the six links did not fall asleep together"
    for s in range(3):
        t.step(100 + s)                                                    # they rest: nothing changes
    assert t.asleep() == list(range(6))
    anchors = np.array([[0.0, 5.0, 0.5, 300.0]], dtype=np.float32)
    t.a.set_pin_anchors([0], anchors)
    assert t.wake_on_b([0]) == list(range(6))                              # pin 0 names body 0: its whole sleeping component
    t.b.set_pin_anchors([0], anchors)
    t.same("after set_pin_anchors")
    assert not t.a.sleep_states()["asleep"].any()
    for s in range(5):
        t.step(200 + s)


# ---- 4. life cycle by twins ------------------------------------------------------------------------------------------------------
def three_columns(units=None):
    """stack(3, 4): three columns of four boxes, three components; with GENEROUS they sleep within a few steps"""
    t = Twins(scenes.stack(3, 4), GENEROUS, lists=units)
    for s in range(6):
        t.step(s)
    assert t.asleep() == list(range(1, 13))
    return t


def column(c):
    return list(range(1 + 4 * c, 5 + 4 * c))


def test_spawn_while_the_world_sleeps():
    t = three_columns()
    px = float(scenes.stack(3, 4)["px"][1])                                 # above column 0
    box = np.array([[px, 75.0, 0.0, 5.0, 5.0]], dtype=np.float32)
    new = t.a.add_bodies(box).tolist()
    assert new == t.b.add_bodies(box).tolist() == [13]
    t.state = sleep_spec.grown(t.state, 14)
    down = np.array([[0.0, -60.0, 0.0]], dtype=np.float32)                  # (faster than the generous tolerance: it does not doze off in the air)
    for w in (t.a, t.b):
        w.set_velocities(new, down)
    t.same("after the spawn")
    assert t.a.sleep_states()[13].tolist() == (0, 0.0, t.b.bodies["inv_mass"][13], t.b.bodies["inv_inertia"][13])
    for s in range(30):
        t.step(s)
        if t.woken[-1]:
            break
    assert t.woken[-1] == column(0), "the box should wake exactly the column it lands on"
    assert t.asleep() == column(1) + column(2)
    for s in range(5):
        t.step(100 + s)


def test_removing_a_sleeper_wakes_its_component_only():
    t = three_columns()
    gone = column(1)[3]
    assert t.wake_on_b([gone]) == column(1)
    remap = t.a.remove_bodies([gone])
    assert remap.tobytes() == t.b.remove_bodies([gone]).tobytes()
    t.state = t.state[remap >= 0].copy()
    t.same("after the removal")
    assert t.asleep() == column(0) + [i - 1 for i in column(2)]
    for s in range(5):
        t.step(s)
    # a removal by box: nobody outside (a true no-op) wakes nobody
    assert t.a.remove_outside([-1e6, -1e6, 1e6, 1e6])[0] == 0
    t.same_states("after the empty removal")


def test_wake_bodies_and_the_calls_that_name_a_body():
    t = three_columns()
    t.a.wake_bodies([column(2)[0], column(2)[1], 0])                        # (twice the same component, and the static ground: fine)
    assert t.wake_on_b([column(2)[0]]) == column(2)
    t.same("after wake_bodies")
    # every per-body call wakes the components of the bodies it names, then does what it does
    for name, args in (("add_accelerations", ([column(0)[1]], np.array([[0.0, 5.0, 0.0]], dtype=np.float32))),
                       ("set_materials", ([column(1)[2]], 0.5, 0.1))):
        getattr(t.a, name)(*args)
        t.wake_on_b(args[0])
        getattr(t.b, name)(*args)
        t.same("after " + name)
    assert t.asleep() == []
    for s in range(6):
        t.step(50 + s)
    assert t.asleep() == list(range(1, 13))
    b = t.b.bodies
    pose = np.array([[b["pos"]["x"][9], b["pos"]["y"][9], b["xv"]["x"][9], b["xv"]["y"][9], b["yv"]["x"][9], b["yv"]["y"][9]]], dtype=np.float32)
    for name, args, wakes in (("set_velocities", ([column(0)[0]], np.array([[1.0, 0.0, 0.0]], dtype=np.float32)), column(0)),
                              ("set_inverse_masses", ([column(1)[1]], np.array([[0.25, 0.5]], dtype=np.float32)), column(1)),
                              ("set_poses", ([9], pose), column(2)),
                              ("set_collision_filters", ([column(0)[2]], 1, 0xFFFFFFFF, 0), [])):      # (column 0 is awake by now)
        getattr(t.a, name)(*args)
        assert t.wake_on_b(args[0]) == wakes, name
        getattr(t.b, name)(*args)
        t.same("after " + name)
    t.a.set_body_flags([column(1)[3]], [0])
    t.b.set_body_flags([column(1)[3]], [0])
    t.flags = True
    t.same("after set_body_flags")
    assert t.asleep() == []
    for s in range(6):
        t.step(s)
    assert t.asleep() == list(range(1, 13))                                 # and they doze off again
    t.a.gravity = -100.0
    t.b.gravity = -100.0
    assert t.wake_everything_on_b() == list(range(1, 13))                   # set_gravity wakes everything
    t.same("after set_gravity")


def test_unit_calls_wake_both_bodies_of_the_units_they_name():
    t = three_columns(units=lists())
    a, b, c = column(0)[3], column(1)[3], column(2)[3]                       # the three columns' top boxes
    pin = pin_rows([(a, b, (5.0, 0.0), (-10.0, 0.0))])
    assert t.a.add_pins(pin).tolist() == [0]
    assert t.wake_on_b([a, b]) == column(0) + column(1)                     # a new unit names both of its bodies
    t.b.add_pins(pin)
    t.same("after add_pins")
    assert t.asleep() == column(2)
    for s in range(8):
        t.step(s)
    assert t.asleep() == list(range(1, 13)), "the pinned pair of columns is one component now and sleeps with the rest"
    assert t.slept[-1] == [] and any(x == column(0) + column(1) for x in t.slept)
    # (with tolerances this generous a body is calm while it still moves, and it freezes where the step's IntegratePosition left it: a
    #  contact it slept with may have no point in the next step, so which of the two columns' boxes still hang together with their
    #  tops is the spec's to say — the twins below hold the device to it — and only the named bodies are certain)
    pair = set(column(0) + column(1))
    t.a.set_break_limits("pin", [0], [1e9])
    woken = set(t.wake_on_b([a, b]))
    assert {a, b} <= woken <= pair
    t.b.set_break_limits("pin", [0], [1e9])
    t.same("after set_break_limits")
    for s in range(8):
        t.step(20 + s)
    assert t.asleep() == list(range(1, 13))
    t.a.remove_pins([0])
    woken = set(t.wake_on_b([a, b]))
    assert {a, b} <= woken <= pair
    t.b.remove_pins([0])
    t.same("after remove_pins")
    assert set(column(2)) <= set(t.asleep()) and not woken & set(t.asleep())
    for s in range(3):
        t.step(40 + s)


def test_turning_sleeping_off_restores_every_mass():
    t = three_columns()
    own = t.a.sleep_states()
    t.a.set_sleeping()
    assert t.a.sleeping() is None
    bodies = t.a.bodies
    assert bodies["inv_mass"].tobytes() == own["inv_mass"].tobytes() and bodies["inv_inertia"].tobytes() == own["inv_inertia"].tobytes()
    t.wake_everything_on_b()
    c = cfg()
    for s in range(4):                                                      # two plain worlds from here on
        t.a.Update(DT, c); t.b.Update(DT, c)
        for x, y in zip(t.a.state(), t.b.state()):
            assert x.tobytes() == y.tobytes()
    assert not t.a.sleep_states()["asleep"].any()


def test_queries_see_a_sleeper_as_a_body_not_as_ground():
    t = three_columns()
    c = phyx_amd.World(0, gravity=G)                                        # the twin whose sleepers were all woken
    c.set_state(*t.b.state())
    own = t.a.sleep_states()
    c.set_inverse_masses(np.arange(1, 13), np.stack([own["inv_mass"][1:], own["inv_inertia"][1:]], axis=1))
    b = t.a.bodies
    boxes = np.stack([b["aabb_min"]["x"], b["aabb_min"]["y"], b["aabb_max"]["x"], b["aabb_max"]["y"]], axis=1)[[0, 1, 6, 12]]
    for x, y in zip(t.a.query_aabb(boxes, skip_static=True), c.query_aabb(boxes, skip_static=True)):
        assert np.array_equal(x, y)
    assert 6 in t.a.query_aabb(boxes[2:3], skip_static=True)[1]
    points = np.stack([b["pos"]["x"], b["pos"]["y"]], axis=1)[[0, 3, 9]]
    assert t.a.query_points(points, skip_static=True).tolist() == c.query_points(points, skip_static=True).tolist() == [-1, 3, 9]
    rays = np.array([[float(b["pos"]["x"][5]), 500.0, 0.0, -1.0, 1000.0]], dtype=np.float32)
    assert t.a.raycast(rays, skip_static=True).tobytes() == c.raycast(rays, skip_static=True).tobytes()
    assert t.a.raycast(rays, skip_static=True)["body"][0] == 8              # the top of column 1, asleep
    named = [1, 2, 7]
    for x, y in zip(t.a.contacts(named, skip_static=True), c.contacts(named, skip_static=True)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert len(t.a.contacts([2], skip_static=True)[1]) > 0                  # box 2 rests on the sleeping box 1 and carries box 3
    assert t.asleep() == list(range(1, 13))                                 # a query names no body: nobody woke


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def snapshot_of(w):
    return tuple(x.tobytes() for x in w.state()) + (w.sleep_states().tobytes(), w.sleeping(), w.sleep_counts())


def test_refusals_leave_the_world_unchanged():
    t = three_columns()
    w = t.a
    before = snapshot_of(w)
    for bad in ((np.nan, 0.05, 0.5), (0.5, np.inf, 0.5), (0.5, 0.05, -1.0), (-0.0001, 0.05, 0.5)):
        with pytest.raises(PhxError) as e:
            w.set_sleeping(*bad)
        assert e.value.status == ERR_INVALID
    with pytest.raises(PhxError) as e:
        w.wake_bodies([99])
    assert e.value.status == ERR_INVALID
    # save and load; an export takes a snapshot, not a world, and no snapshot of such a world can come to exist: fork is save + load
    snap = phyx_amd.api.Snapshot(0)
    plain = phyx_amd.World(0, gravity=G)
    plain.add_scene(scenes.stack(2, 2))
    filled = plain.save()
    for call in (lambda: w.save(snap), lambda: w.load(filled), w.fork):
        with pytest.raises(PhxError) as e:
            call()
        assert e.value.status == ERR_STATE and "sleep" in str(e.value)
    with pytest.raises(PhxError) as e:
        snap.counts                                                         # nothing was saved into it: never filled
    assert e.value.status == ERR_STATE
    # a sharded world carries no sleep states, and a sleeping world does not become one
    with pytest.raises(PhxError) as e:
        w.set_shard(0, 2)
    assert e.value.status == ERR_STATE and "sleep" in str(e.value)
    assert snapshot_of(w) == before
    # mid-step
    w.PreSolve(DT)
    for call in (lambda: w.set_sleeping(0.5, 0.05, 0.5), w.set_sleeping, lambda: w.wake_bodies([1]), w.sleep_states, w.sleep_counts):
        with pytest.raises(PhxError) as e:
            call()
        assert e.value.status == ERR_STATE
    w.FinishStep(DT, t.cfg)
    t.b.Update(DT, t.cfg)
    t.same("after the refused calls")
    # the other way round: a sharded world refuses sleeping
    s = phyx_amd.World(0, gravity=G)
    s.add_scene(scenes.stack(2, 2))
    s.set_shard(0, 2)
    with pytest.raises(PhxError) as e:
        s.set_sleeping(0.5, 0.05, 0.5)
    assert e.value.status == ERR_STATE
    assert s.sleeping() is None


def test_a_world_that_never_enabled_it_reports_nobody_asleep():
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scenes.stack(2, 3))
    w.Update(DT, cfg())
    st = w.sleep_states()
    b = w.bodies
    assert not st["asleep"].any() and not st["timer"].any()
    assert st["inv_mass"].tobytes() == b["inv_mass"].tobytes() and st["inv_inertia"].tobytes() == b["inv_inertia"].tobytes()
    assert w.sleep_counts() == (0, 0, 0) and w.sleeping() is None
    w.wake_bodies([1])                                                      # nothing to do
    w.set_sleeping()                                                        # off already


def test_set_state_resets_the_column_and_keeps_the_parameters():
    t = three_columns()
    state = t.b.state()
    t.a.set_state(*state)
    assert t.a.sleeping() == tuple(float(np.float32(x)) for x in GENEROUS)
    assert not t.a.sleep_states()["asleep"].any() and t.a.sleep_counts() == (0, 0, 0)
    # the restored bodies are the statics B shows; nobody holds their masses any more: that is what set_state of such a state means
    assert t.a.bodies.tobytes() == state[0].tobytes()


# ---- 6. no extra host wait ---------------------------------------------------------------------------------------------------------
def test_a_sleeping_world_waits_no_more_often_than_a_plain_one():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sleep_wait_worker.py")
    p = subprocess.run([sys.executable, worker], env=dict(os.environ, PHX_WAIT_CLOCK="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print(got)
    assert got["asleep"] == got["mobile"] > 0
    assert got["waits_off"] > 0
    assert got["waits_on"] == got["waits_off"], got
