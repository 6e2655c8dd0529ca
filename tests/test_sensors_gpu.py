"""Body flags and sensors (phx_world_set_body_flags) on the device, held to tests/sensor_spec.py and to the oracle:
  - the per-step pin: before each step an unflagged tag twin T = set_state(F's state, joints tagged) shows what RefreshContactJoints was
    entered with; F's joints and solver_index are sensor_spec.refresh of that under F's flags, its manifolds and contact points T's, and
    its solve the oracle's on its own schedule;
  - an active column that flags nothing is the plain world, in lockstep with the oracle World;
  - dynamic sensors fall freely, begin and end touch events, and report contacts without joints;
  - a flag set on a settled stack takes exactly that box's joints at the next step and gives them back, cold, when it is cleared;
  - the schedule rebuild of a flagged world is the same with PHX_NO_PRELABEL=1 and without;
  - flags move with removals and spawns, set_state resets them, and the calls are refused where the header says so;
  - examples/trigger.c builds and passes its own checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contact_spec
import phyx_amd
import sensor_spec as spec
from helpers import oracle_world
from phyx_amd import Configuration, scenes
from phyx_amd.api import CONTACT_NO_JOINT, rigid_body_dtype
from spawn_lockstep import compare, step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1.0 / 60.0
G = -200.0
NAMES = ("bodies", "manifolds", "contact points", "joints")


def _cfg(mode, iters=15):
    return Configuration(phyx_amd.SOLVE_AVX2, mode, iters, iters)


def _world(scene, gravity=G):
    pw = phyx_amd.World(0, gravity=gravity)
    pw.add_scene(scene)
    return pw


def _same(a, b, what):
    assert a.counts() == b.counts(), "counts differ %s" % what
    for name, x, y in zip(NAMES, a.state(), b.state()):
        assert x.tobytes() == y.tobytes(), "%s differ %s" % (name, what)


def _fifth(n):
    """Every fifth non-ground body a sensor."""
    f = spec.defaults(n)
    f[5::5] = spec.BODY_SENSOR
    return f


# ---- the per-step pin ------------------------------------------------------------------------------------------------------------------
def _pin_step(oracle, pf, flags, cfg, s, tally):
    """One step of the flagged world F against its unflagged tag twin T, sensor_spec.refresh and the oracle's solver."""
    b0, m0, c0, j0 = pf.state()
    tagged = j0.copy()
    tagged["friction_acc"] = spec.tags(len(j0))
    pt = phyx_amd.World(0, gravity=G)
    pt.set_state(b0, m0, c0, tagged)                                        # (set_state resets the flags: T is the plain world)
    pf.PreSolve(DT)
    pt.PreSolve(DT)
    mf, mt = pf.manifolds, pt.manifolds
    assert mf.tobytes() == mt.tobytes(), "step %d: manifolds differ from the twin's" % s
    cf, ct = pf.contactPoints, pt.contactPoints
    x, y = cf.copy(), ct.copy()
    x["solver_index"], y["solver_index"] = 0, 0
    assert x.tobytes() == y.tobytes(), "step %d: contact points differ from the twin's in more than solver_index" % s
    recon, _ = spec.tag_twin_reconstruct(mt, ct, pt.contactJoints, ct)
    st = {}
    want_cps, want_joints = spec.refresh(mf, recon, j0, flags, st)
    jf = pf.contactJoints
    assert jf.tobytes() == want_joints.tobytes(), "step %d: joints differ from sensor_spec.refresh" % s
    assert cf["solver_index"].tobytes() == want_cps["solver_index"].tobytes(), "step %d: solver_index differs from sensor_spec.refresh" % s
    tally["sensor_slots"] += len(spec.sensor_slots(flags, mf))
    tally["dead_and_new"] += st["created"] > 0 and st["deleted"] > 0
    b = pf.bodies
    pf.FinishStep(DT, cfg)
    order, offs = pf.solver.schedule()
    groups, _ = pf.solver.groups()
    assert len(order) == len(jf)
    ob, oj = b.view(oracle.body_dtype).copy(), jf.view(oracle.joint_dtype).copy()
    oracle.solver_solve_grouped(ob, cf.view(oracle.contact_point_dtype), oj, order, offs, groups, cfg.contactIterationsCount,
                                cfg.penetrationIterationsCount, oracle.STAG_COLOUR_SYNC)
    assert pf.contactJoints.tobytes() == oj.tobytes(), "step %d: impulses differ from the oracle's" % s
    got, want = pf.bodies, ob.view(rigid_body_dtype)
    assert got["velocity"].tobytes() == want["velocity"].tobytes(), "step %d: velocities differ" % s
    assert got["angular_velocity"].tobytes() == want["angular_velocity"].tobytes(), "step %d: angular velocities differ" % s


def _pin_scene(name):
    if name == "piles":
        sc = scenes.piles(3, 60, ymax=260.0)
        pf = _world(sc)
        flags = _fifth(len(sc["px"]))
        return pf, flags, _cfg(phyx_amd.ISLAND_MULTIPLE_SLOPPY)
    sc = scenes.stack(4, 12)
    pf = _world(sc)
    zone = pf.AddBody((0.0, 40.0), 0.0, (40.0, 8.0), static=True)           # a fixed trigger zone across all four columns, as the last body
    flags = spec.defaults(zone + 1)
    flags[zone] = spec.BODY_SENSOR
    return pf, flags, _cfg(phyx_amd.ISLAND_SINGLE)


@pytest.mark.parametrize("name", ["piles", "stack_zone"])
def test_per_step_pin(oracle, built_lib, name):
    """Scene 1: piles(3, 60, ymax=260) with every fifth non-ground body a sensor, MULTIPLE_SLOPPY; scene 2: stack(4, 12) with a static
    sensor box as the last body, SINGLE.  40 steps each; some step has sensor slots, and in scene 1 some refresh deletes and creates
    joints together."""
    pf, flags, cfg = _pin_scene(name)
    pf.set_body_flags(np.flatnonzero(flags).astype(np.int32), spec.BODY_SENSOR)
    assert (pf.body_flags() == flags).all()
    tally = {"sensor_slots": 0, "dead_and_new": 0}
    for s in range(40):
        _pin_step(oracle, pf, flags, cfg, s, tally)
    assert (pf.body_flags() == flags).all()
    assert tally["sensor_slots"] > 0, "no step had a sensor slot"
    if name == "piles":
        assert tally["dead_and_new"] > 0, "no refresh had dead and new joints together"
    assert pf.counts()[3] > 0
    assert pf.build_counts()[0] == 0, "a flagged world's rebuild took its components from the manifolds"


# ---- an active column that flags nothing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack", "piles"])
def test_active_column_that_flags_nothing(oracle, built_lib, name):
    """Every flag set to 0 (before the first step on the stack; after five steps, on the device, on the piles): the sensor kernels run
    and find no sensor — bit-exact lockstep with the oracle World for 40 steps."""
    sc = scenes.stack(4, 12) if name == "stack" else scenes.piles(3, 50, ymax=220.0)
    cfg = _cfg(phyx_amd.ISLAND_MULTIPLE_SLOPPY)
    pw, ow = _world(sc), oracle_world(sc)
    n = len(sc["px"])
    at = 0 if name == "stack" else 5
    for s in range(40):
        if s == at:
            pw.set_body_flags(np.arange(n, dtype=np.int32), 0)
            assert (pw.body_flags() == 0).all()
        step(oracle, pw, ow, cfg, DT)
        compare(pw, ow, s)
    assert len(ow.joints()) > 0


# ---- dynamic sensors ------------------------------------------------------------------------------------------------------------------
def test_dynamic_sensors_fall_freely_and_report(oracle, built_lib):
    """Six sensor boxes inside stack(4, 12): 60 steps; their records are the oracle World of the six alone but for `index`, some sensor
    pair begins and later ends, and the sensors' contacts are contact_spec's over the getters, all without joints."""
    cfg = _cfg(phyx_amd.ISLAND_MULTIPLE_SLOPPY)
    sc = scenes.stack(4, 12)
    n = len(sc["px"])
    boxes = [(-22.5 + 15.0 * k, 40.0 + 12.0 * k, 0.1 * k, 4.0, 3.0) for k in range(6)]      # inside the pile, 15 apart in x
    pw = _world(sc)
    for x, y, a, hx, hy in boxes:
        pw.AddBody((x, y), a, (hx, hy))
    sensors = np.arange(n, n + len(boxes), dtype=np.int32)
    pw.set_body_flags(sensors, spec.BODY_SENSOR)
    og = oracle.OracleWorld(G)
    for x, y, a, hx, hy in boxes:
        og.add_body(x, y, a, hx, hy)
    began, ended_after_begin, records = {}, 0, 0
    for s in range(60):
        pw.Update(DT, cfg)
        og.update(DT)
        g, want = pw.bodies[n:].copy(), og.bodies().copy()
        g["index"] = 0
        want["index"] = 0
        assert g.tobytes() == want.tobytes(), "sensors differ from free fall at step %d" % s
        begin, end = pw.contact_events()
        for a, b in begin.tolist():
            if a >= n or b >= n:
                began.setdefault((a, b), s)
        for a, b in end.tolist():
            if (a, b) in began and began[(a, b)] < s:
                ended_after_begin += 1
        bodies, manifolds, cps, joints = pw.state()
        offsets, got = pw.contacts(sensors)
        want_offsets, want_records = contact_spec.contacts(bodies, manifolds, cps, joints, sensors)
        assert offsets.tobytes() == want_offsets.tobytes() and got.tobytes() == want_records.tobytes(), "contacts differ at step %d" % s
        assert ((got["flags"] & CONTACT_NO_JOINT) != 0).all() and (got["normal_impulse"] == 0).all() and (got["friction_impulse"] == 0).all(), "step %d" % s
        records += len(got)
        sens = spec.sensor_manifolds(pw.body_flags(), manifolds)
        assert (cps["solver_index"][spec.live_slots(manifolds[sens])] == -1).all()
    assert records > 0 and began and ended_after_begin > 0
    start = np.array([b[1] for b in boxes], dtype=np.float32)
    assert (pw.bodies["pos"]["y"][n:] < start - 50.0).all(), "the sensors did not fall through the stack"


# ---- toggle ---------------------------------------------------------------------------------------------------------------------------
def _settled_stack(steps=60):
    cfg = _cfg(phyx_amd.ISLAND_SINGLE)
    pw = _world(scenes.stack(6, 10))
    for _ in range(steps):
        pw.Update(DT, cfg)
    return pw, cfg


def test_toggle(built_lib):
    """A settled stack(6, 10), one mid-stack box flagged: the call changes nothing but the flag; the next step's refresh holds exactly that
    box's live slots fewer joints than an unflagged twin's and the schedule is rebuilt; cleared, the joints come back with zero impulses."""
    pw, cfg = _settled_stack()
    box = 1 + 2 * 10 + 4                                                     # column 2, row 4: a box above and a box below
    before = pw.state()
    nj = pw.counts()[3]
    pw.set_body_flags([box], spec.BODY_SENSOR)
    assert pw.counts() == tuple(len(x) for x in before), "the call itself changed the counts"
    for x, y in zip(before, pw.state()):
        assert x.tobytes() == y.tobytes(), "the call itself changed the state"
    twin = phyx_amd.World(0, gravity=G)
    twin.set_state(*before)
    pw.PreSolve(DT)
    twin.PreSolve(DT)
    m = pw.manifolds
    assert m.tobytes() == twin.manifolds.tobytes()
    mine = (m["body1"] == box) | (m["body2"] == box)
    slots = int(m["point_count"][mine].sum())
    assert slots >= 2
    assert pw.counts()[3] == twin.counts()[3] - slots and pw.counts()[3] < nj, "the box's joints, and only they, did not go"
    assert (pw.contactPoints["solver_index"][spec.live_slots(m[mine])] == -1).all()
    pw.FinishStep(DT, cfg)
    assert pw.solver.stats().recoloured == 1
    # clear the flag: the joints come back cold
    pw.set_body_flags([box], 0)
    pw.PreSolve(DT)
    m, cps, joints = pw.manifolds, pw.contactPoints, pw.contactJoints
    mine = (m["body1"] == box) | (m["body2"] == box)
    back = cps["solver_index"][spec.live_slots(m[mine])]
    assert len(back) >= 2 and (back >= 0).all()
    assert (joints["body1"][back] == box).any() and (joints["body2"][back] == box).any()
    assert (joints["normal_acc"][back] == 0).all() and (joints["friction_acc"][back] == 0).all(), "the returning joints are not cold"
    assert (joints["normal_acc"] != 0).any()
    pw.FinishStep(DT, cfg)
    assert pw.solver.stats().recoloured == 1


def test_flag_on_a_body_without_manifold_keeps_the_schedule(built_lib):
    cfg = _cfg(phyx_amd.ISLAND_SINGLE)
    pw = _world(scenes.stack(6, 10), gravity=0.0)
    loner = pw.AddBody((900.0, 300.0), 0.0, (5.0, 5.0))
    seen = []
    for _ in range(60):
        pw.Update(DT, cfg)
        seen.append(pw.solver.stats().recoloured)
        if seen[-3:] == [0, 0, 0]:
            break
    assert seen[-3:] == [0, 0, 0], seen
    m = pw.manifolds
    assert not ((m["body1"] == loner) | (m["body2"] == loner)).any()
    pw.set_body_flags([loner], spec.BODY_SENSOR)
    pw.Update(DT, cfg)
    assert pw.solver.stats().recoloured == 0, "a flag on a body in no manifold rebuilt the schedule"


# ---- the manifold-side rebuild ------------------------------------------------------------------------------------------------------------
def test_rebuild_is_the_same_without_prelabel(built_lib):
    """Scene 1 of the pin, 20 steps, in a world created with PHX_NO_PRELABEL=1 and in one created without: all four arrays byte-equal
    every step."""
    sc = scenes.piles(3, 60, ymax=260.0)
    flags = _fifth(len(sc["px"]))
    cfg = _cfg(phyx_amd.ISLAND_MULTIPLE_SLOPPY)
    had = os.environ.get("PHX_NO_PRELABEL")
    try:
        os.environ["PHX_NO_PRELABEL"] = "1"
        pa = _world(sc)
        os.environ.pop("PHX_NO_PRELABEL")
        pb = _world(sc)
    finally:
        if had is None:
            os.environ.pop("PHX_NO_PRELABEL", None)
        else:
            os.environ["PHX_NO_PRELABEL"] = had
    for pw in (pa, pb):
        pw.set_body_flags(np.flatnonzero(flags).astype(np.int32), spec.BODY_SENSOR)
    for s in range(20):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "at step %d" % s)
    assert pa.counts()[3] > 0 and len(spec.sensor_slots(flags, pa.manifolds)) > 0


# ---- carry and refuse -------------------------------------------------------------------------------------------------------------------
def test_flags_survive_removal_and_spawn(built_lib):
    pw, cfg = _settled_stack(steps=10)
    n = pw.counts()[0]
    rng = np.random.default_rng(4)
    f = (rng.random(n) < 0.3).astype(np.uint32)
    pw.set_body_flags(np.arange(n, dtype=np.int32), f)
    remap = pw.remove_bodies(np.array([2, 9, 30], dtype=np.int32))
    f = spec.remove(f, remap >= 0)
    assert (pw.body_flags() == f).all(), "flags did not move with the kept bodies"
    rows = np.array([[900.0 + 20.0 * k, 50.0, 0.0, 5.0, 5.0] for k in range(4)], dtype=np.float32)
    pw.add_bodies(rows)
    f = spec.spawn(f, 4)
    assert (pw.body_flags() == f).all()
    pw.Update(DT, cfg)
    m, cps = pw.manifolds, pw.contactPoints
    assert (cps["solver_index"][spec.sensor_slots(f, m)] == -1).all()
    assert (cps["solver_index"][spec.live_slots(m[~spec.sensor_manifolds(f, m)])] >= 0).all()
    pw.AddBody((-900.0, 50.0), 0.0, (5.0, 5.0))                              # host-staged again: flags come along
    f = spec.spawn(f, 1)
    assert (pw.body_flags() == f).all()
    pw.Update(DT, cfg)
    assert (pw.body_flags() == f).all()


def test_set_state_then_flags_is_a_twin(built_lib):
    pa, cfg = _settled_stack(steps=20)
    n = pa.counts()[0]
    f = _fifth(n)
    idx = np.flatnonzero(f).astype(np.int32)
    pa.set_body_flags(idx, spec.BODY_SENSOR)
    for _ in range(10):
        pa.Update(DT, cfg)
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*pa.state())
    assert (pb.body_flags() == spec.set_state(n)).all(), "set_state did not reset the flags"
    pb.set_body_flags(idx, spec.BODY_SENSOR)
    for s in range(10):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "after step %d" % s)


def test_rejections_leave_the_world_unchanged(built_lib):
    pw, cfg = _settled_stack(steps=10)
    L, n = built_lib, pw.counts()[0]
    pw.set_body_flags([4], spec.BODY_SENSOR)
    before, fbefore = pw.state(), pw.body_flags()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    f = np.array([1, 0], dtype=np.uint32)
    i = np.array([1, 2], dtype=np.int32)
    for bad in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert L.phx_world_set_body_flags(pw.h, vp(i), vp(np.array([1, bad], dtype=np.uint32)), 2) == -1
    assert not spec.valid([2, 3, 0x80000000, 0xFFFFFFFE]).any()
    for idx in ([0, n], [-1, 3], [5, 5]):
        assert L.phx_world_set_body_flags(pw.h, vp(np.array(idx, dtype=np.int32)), vp(f), 2) == -1
    assert L.phx_world_set_body_flags(pw.h, vp(i), vp(f), -1) == -1
    assert L.phx_world_set_body_flags(pw.h, None, vp(f), 2) == -1
    assert L.phx_world_set_body_flags(pw.h, vp(i), None, 2) == -1
    out = np.zeros(n - 1, dtype=np.uint32)
    assert L.phx_world_get_body_flags(pw.h, vp(out), n - 1) == -4
    pw.PreSolve(DT)
    assert L.phx_world_set_body_flags(pw.h, vp(i), vp(f), 2) == -5
    pw.FinishStep(DT, cfg)
    twin = phyx_amd.World(0, gravity=G)
    twin.set_state(*before)
    twin.set_body_flags([4], spec.BODY_SENSOR)
    twin.Update(DT, cfg)
    _same(pw, twin, "after the refused calls and a step")
    assert (pw.body_flags() == fbefore).all()


def test_sharded_worlds_refuse(built_lib):
    L = built_lib
    pw = _world(scenes.stack(2, 3))
    pw.set_shard(0, 2)
    i, f = np.array([1], dtype=np.int32), np.array([1], dtype=np.uint32)
    assert L.phx_world_set_body_flags(pw.h, i.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), 1) == -5
    pw.set_shard(0, 1)
    pw.set_body_flags(i, spec.BODY_SENSOR)
    assert L.phx_world_set_shard(pw.h, 0, 2) == -5                        # a flag is set: no sharding
    pw.set_body_flags(i, 0)                                                # cleared: allowed again
    assert L.phx_world_set_shard(pw.h, 0, 2) == 0


# ---- the example ------------------------------------------------------------------------------------------------------------------------
def test_trigger_example_runs(tmp_path, built_lib):
    exe = str(tmp_path / "trigger")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "trigger.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    r = subprocess.run([exe, "240"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for box in (1, 2, 3):
        assert "box %d enters the zone" % box in r.stdout and "box %d has left the zone" % box in r.stdout
    assert "the same poses, bit for bit" in r.stdout
