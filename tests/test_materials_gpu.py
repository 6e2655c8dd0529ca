"""Materials (phx_world_set_materials) on the device, held to tests/material_spec.py and to the oracle World:
  - every material set explicitly to the default: lockstep with the oracle World byte for byte, in Single (the HBM colour path, and a
    wall whose component is partitioned: k_solve_parts / k_solve_tail) and Multiple Sloppy (the LDS islands);
  - mixed materials (ice, rubber, fast drops): every step the oracle World's pre_solve, material_spec.solve_grouped on the device's
    schedule, the oracle's integrate_position, byte for byte; materials changed mid-run;
  - behaviour: a box on ice keeps sliding, on friction 1 it stops; a rubber box bounces, a default one does not;
  - bookkeeping: removal, spawn, set_state, filters and edits; the schedule stays; rejections; sharding; queries and contact reports;
  - the cfg 2 world with every material the default, three steps against an untouched twin."""
import ctypes as C

import numpy as np
import pytest

import material_spec as spec
import phyx_amd
from helpers import oracle_world
from phyx_amd import Configuration, scenes
from spawn_lockstep import compare, step

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
NAMES = ("bodies", "manifolds", "contact points", "joints")
MODES = {"single": phyx_amd.ISLAND_SINGLE, "multiple_sloppy": phyx_amd.ISLAND_MULTIPLE_SLOPPY}


def _cfg(mode, iters=15):
    return Configuration(phyx_amd.SOLVE_AVX2, MODES[mode], iters, iters)


def _world(scene, gravity=G):
    pw = phyx_amd.World(0, gravity=gravity)
    pw.add_scene(scene)
    return pw


def _same(a, b, what):
    assert a.counts() == b.counts(), "counts differ %s" % what
    for name, x, y in zip(NAMES, a.state(), b.state()):
        assert x.tobytes() == y.tobytes(), "%s differ %s" % (name, what)


def _all(pw):
    return np.arange(pw.counts()[0], dtype=np.int32)


# ---- 1. active defaults ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["single", "multiple_sloppy"])
@pytest.mark.parametrize("when", ["before_first_step", "after_five_steps"])
def test_active_defaults_lockstep(oracle, built_lib, mode, when):
    """Every body given {0.3, 0} (the material kernels run, every pair value the reference's constant): 40 steps byte for byte with the
    oracle World replaying the device's schedule."""
    cfg = _cfg(mode)
    sc = scenes.stack(4, 12) if when == "before_first_step" else scenes.stack(6, 8)
    pw, ow = _world(sc), oracle_world(sc)
    for s in range(40):
        if s == (0 if when == "before_first_step" else 5):
            pw.set_materials(_all(pw), 0.3, 0.0)
            assert (pw.materials() == spec.defaults(pw.counts()[0])).all()
        step(oracle, pw, ow, cfg, DT)
        compare(pw, ow, s)


def test_active_defaults_partitioned_wall(oracle, built_lib):
    """A wall whose one component has more than 1024 joints (the HBM group, partitioned: k_solve_parts_ahead_mat / k_solve_parts_mat /
    k_solve_tail_mat), every material the default: 12 steps byte for byte with the oracle World."""
    cfg = _cfg("single")
    sc = scenes.wall(20, 30)
    pw, ow = _world(sc), oracle_world(sc)
    pw.set_materials(_all(pw), 0.3, 0.0)
    parts = 0
    for s in range(12):
        step(oracle, pw, ow, cfg, DT)
        compare(pw, ow, s)
        parts = max(parts, pw.solver.partition()[1])
    assert pw.counts()[3] > 1024
    assert parts > 0, "the wall's component was not partitioned"


# ---- 2. mixed materials ----------------------------------------------------------------------------------------------------------------
def _mixed(n, seed):
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 4, n)                      # 0 default, 1 ice, 2 rubber, 3 rough
    f = np.choose(kind, [0.3, 0.0, 0.8, 1.0]).astype(np.float32)
    e = np.choose(kind, [0.0, 0.0, 0.8, 0.2]).astype(np.float32)
    return spec.materials(n, f, e)


def _spec_step(oracle, pw, ow, cfg, mat):
    """pw.Update and the oracle World's step with material_spec's solve on the device's schedule.  Returns the largest dstVelocity the
    refresh of this step computed (a joint really bounced if > 0)."""
    pw.Update(DT, cfg)
    ow.pre_solve(DT)
    order, offs = pw.solver.schedule()
    groups, _ = pw.solver.groups()
    b, cp, j = ow.bodies(), ow.contact_points(), ow.joints()
    assert len(order) == len(j)
    mu, e = spec.joint_values(mat, j)
    top = spec.max_dst_velocity(b, cp, j, e)
    spec.solve_grouped(b, cp, j, order, offs, groups, cfg.contactIterationsCount, cfg.penetrationIterationsCount, mu, e,
                       fused=oracle.get_arith())
    ow.integrate_position(DT)
    return top


@pytest.mark.parametrize("mode", ["single", "multiple_sloppy"])
def test_mixed_materials_follow_the_spec(oracle, built_lib, mode):
    """Ice, rubber, rough and default bodies, and four boxes dropped fast onto the stacks: 40 steps byte for byte with the oracle World
    under material_spec's solve; at step 20 the materials change (rubber everywhere but the ground)."""
    cfg = _cfg(mode)
    sc = scenes.stack(4, 10)
    pw, ow = _world(sc), oracle_world(sc)
    for k in range(4):
        x = -22.5 + 15.0 * k
        pw.AddBody((x, 400.0 + 30.0 * k), 0.05 * k, (4.0, 4.0))
        ow.add_body(x, 400.0 + 30.0 * k, 0.05 * k, 4.0, 4.0)
    n = pw.counts()[0]
    mat = _mixed(n, 1)
    pw.set_materials(_all(pw), mat["friction"], mat["restitution"])
    bounced = 0.0
    for s in range(40):
        if s == 20:
            mat = spec.materials(n, 0.6, 0.9)
            mat[0] = spec.defaults(1)[0]
            pw.set_materials(_all(pw), mat["friction"], mat["restitution"])
        bounced = max(bounced, _spec_step(oracle, pw, ow, cfg, mat))
        compare(pw, ow, s)
    assert (pw.materials() == mat).all()
    assert bounced > 0, "no joint got dstVelocity > 0: the restitution path was not exercised"


def test_mixed_materials_partitioned_wall(oracle, built_lib):
    """The partitioned wall with mixed materials: 8 steps byte for byte under material_spec's solve."""
    cfg = _cfg("single")
    sc = scenes.wall(20, 30)
    pw, ow = _world(sc), oracle_world(sc)
    mat = _mixed(pw.counts()[0], 2)
    pw.set_materials(_all(pw), mat["friction"], mat["restitution"])
    for s in range(8):
        _spec_step(oracle, pw, ow, cfg, mat)
        compare(pw, ow, s)
    assert pw.solver.partition()[1] > 0


# ---- 3. behaviour ----------------------------------------------------------------------------------------------------------------------
def _slider(friction):
    pw = phyx_amd.World(0, gravity=G)
    pw.AddBody((0.0, 0.0), 0.0, (2000.0, 10.0), static=True)
    box = pw.AddBody((-1500.0, 14.9), 0.0, (5.0, 5.0))
    pw.set_materials(np.array([0, box], dtype=np.int32), friction, 0.0)
    cfg = _cfg("single")
    for _ in range(10):                                # settle on the ground
        pw.Update(DT, cfg)
    pw.set_velocities(np.array([box], dtype=np.int32), np.array([[50.0, 0.0, 0.0]], dtype=np.float32))
    v0 = float(pw.bodies[box]["velocity"]["x"])
    for _ in range(60):
        pw.Update(DT, cfg)
    return v0, float(pw.bodies[box]["velocity"]["x"]), pw.counts()[1]


def test_ice_slides_rough_stops(built_lib):
    v0, v, nm = _slider(0.0)
    assert nm > 0 and v0 == 50.0
    assert abs(v - v0) < 1e-3, "a box on ice lost %g of its speed" % (v0 - v)
    v0, v, _ = _slider(1.0)
    assert abs(v) < 1e-2, "a box on friction 1 still moves at %g" % v


def _drop(restitution):
    pw = phyx_amd.World(0, gravity=G)
    pw.AddBody((0.0, 0.0), 0.0, (100.0, 10.0), static=True)
    box = pw.AddBody((0.0, 200.0), 0.0, (5.0, 5.0))
    pw.set_materials(np.array([box], dtype=np.int32), 0.3, restitution)
    cfg = _cfg("single")
    vy = []
    for _ in range(120):
        pw.Update(DT, cfg)
        vy.append(float(pw.bodies[box]["velocity"]["y"]))
    vy = np.array(vy)
    k = int(np.argmax(vy > -1e-3)) if (vy > -1e-3).any() else len(vy)
    impact = -float(vy[:k].min()) if k else 0.0
    return impact, float(vy.max())


def test_rubber_bounces_default_does_not(built_lib):
    impact, up = _drop(0.8)
    assert impact > 100.0
    assert up > 0.5 * impact, "rubber rose at %g after an impact at %g" % (up, impact)
    impact, up = _drop(0.0)
    assert up < 5.0, "a default box bounced at %g" % up


# ---- 4. bookkeeping --------------------------------------------------------------------------------------------------------------------
def _settled(steps=10, mode="single"):
    pw = _world(scenes.stack(4, 12))
    cfg = _cfg(mode)
    for _ in range(steps):
        pw.Update(DT, cfg)
    return pw, cfg


def test_removal_spawn_set_state_filters_edits(built_lib):
    pw, cfg = _settled()
    n = pw.counts()[0]
    mat = _mixed(n, 3)
    pw.set_materials(_all(pw), mat["friction"], mat["restitution"])
    remap = pw.remove_bodies(np.array([2, 9, 30], dtype=np.int32))
    mat = spec.remove(mat, remap >= 0)
    assert (pw.materials() == mat).all(), "materials did not move with the kept bodies"
    pw.add_bodies(np.array([[900.0 + 20.0 * k, 50.0, 0.0, 5.0, 5.0] for k in range(4)], dtype=np.float32))
    mat = spec.spawn(mat, 4)
    assert (pw.materials() == mat).all()
    pw.Update(DT, cfg)
    pw.AddBody((-900.0, 50.0), 0.0, (5.0, 5.0))        # host-staged again: the table comes along
    mat = spec.spawn(mat, 1)
    assert (pw.materials() == mat).all()
    pw.Update(DT, cfg)
    k = pw.counts()[0]
    pw.set_collision_filters(np.array([3], dtype=np.int32), mask=0)
    pw.set_velocities(np.array([5], dtype=np.int32), np.array([[1.0, 2.0, 0.5]], dtype=np.float32))
    pw.set_inverse_masses(np.array([6], dtype=np.int32), np.array([[0.5, 0.01]], dtype=np.float32))
    assert (pw.materials() == mat).all() and len(mat) == k, "filters or edits touched the materials"
    pw.Update(DT, cfg)
    assert (pw.materials() == mat).all()
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*pw.state())
    assert (pb.materials() == spec.defaults(k)).all()
    pw.set_state(*pw.state())
    assert (pw.materials() == spec.set_state(k)).all(), "set_state did not reset the materials"


def test_set_state_then_materials_is_a_twin(built_lib):
    pa, cfg = _settled(steps=20, mode="multiple_sloppy")
    n = pa.counts()[0]
    mat = _mixed(n, 4)
    pa.set_materials(_all(pa), mat["friction"], mat["restitution"])
    for _ in range(5):
        pa.Update(DT, cfg)
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*pa.state())
    pb.set_materials(_all(pb), mat["friction"], mat["restitution"])
    for s in range(10):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "after step %d" % s)


def test_material_change_keeps_the_schedule(built_lib):
    pw = _world(scenes.stack(4, 12), gravity=0.0)
    cfg = _cfg("single")
    seen = []
    for _ in range(60):
        pw.Update(DT, cfg)
        seen.append(pw.solver.stats().recoloured)
        if seen[-3:] == [0, 0, 0]:
            break
    assert seen[-3:] == [0, 0, 0], seen
    pw.set_materials(_all(pw)[1:], 0.05, 0.5)
    pw.Update(DT, cfg)
    assert pw.solver.stats().recoloured == 0, "a change of materials rebuilt the schedule"


def test_rejections_leave_the_world_unchanged(built_lib):
    pw, cfg = _settled()
    L, n = built_lib, pw.counts()[0]
    pw.set_materials(np.array([4], dtype=np.int32), 0.7, 0.25)
    before, mbefore = pw.state(), pw.materials()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    good = spec.materials(2, 0.5, 0.5)
    for idx in ([0, n], [-1, 3], [5, 5]):
        i = np.array(idx, dtype=np.int32)
        assert L.phx_world_set_materials(pw.h, vp(i), vp(good), 2) == -1
    i = np.array([1, 2], dtype=np.int32)
    for f, e in ((-0.1, 0.0), (1.5e6, 0.0), (np.nan, 0.0), (np.inf, 0.0), (0.3, -0.01), (0.3, 1.01), (0.3, np.nan), (0.3, np.inf)):
        bad = spec.materials(2, [0.5, f], [0.5, e])
        assert L.phx_world_set_materials(pw.h, vp(i), vp(bad), 2) == -1, (f, e)
    assert L.phx_world_set_materials(pw.h, vp(i), vp(good), -1) == -1
    assert L.phx_world_set_materials(pw.h, None, vp(good), 2) == -1
    assert L.phx_world_set_materials(pw.h, vp(i), None, 2) == -1
    out = np.zeros(n - 1, dtype=good.dtype)
    assert L.phx_world_get_materials(pw.h, vp(out), n - 1) == -4
    with pytest.raises(phyx_amd.PhxError):
        pw.set_materials(i, 0.3, 2.0)
    pw.PreSolve(DT)
    assert L.phx_world_set_materials(pw.h, vp(i), vp(good), 2) == -5
    pw.FinishStep(DT, cfg)
    assert (pw.materials() == mbefore).all()
    twin = phyx_amd.World(0, gravity=G)
    twin.set_state(*before)
    twin.set_materials(np.array([4], dtype=np.int32), 0.7, 0.25)
    twin.Update(DT, cfg)
    _same(pw, twin, "after the refused calls and a step")


def test_sharded_worlds_and_fp16_refuse(built_lib):
    L = built_lib
    pw = _world(scenes.stack(2, 3))
    pw.set_shard(0, 2)
    i, m = np.array([1], dtype=np.int32), spec.materials(1, 0.0, 0.0)
    assert L.phx_world_set_materials(pw.h, i.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), 1) == -5
    pw.set_shard(0, 1)
    pw.set_materials(i, 0.0, 0.0)
    assert L.phx_world_set_shard(pw.h, 0, 2) == -5                        # a non-default material: no sharding
    pw.set_materials(i, 0.3, 0.0)                                          # back to the default: allowed again
    assert L.phx_world_set_shard(pw.h, 0, 2) == 0
    pw.set_shard(0, 1)
    # the fp16 ablation refuses a step of a world with materials
    pw = _world(scenes.stack(2, 3))
    pw.set_materials(i, 0.5, 0.5)
    assert L.phx_solver_set_body_state_bits(L.phx_world_solver(pw.h), 16) == 0
    cfg = _cfg("multiple_sloppy")._c()
    assert L.phx_world_update(pw.h, C.c_float(DT), C.byref(cfg)) == -5


def test_queries_and_contacts_as_a_twin(built_lib):
    """A world with materials answers queries and contact reports like a twin without them: same state, same answers."""
    pa, cfg = _settled(steps=5)
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*pa.state())
    pa.set_materials(_all(pa), 0.9, 0.4)
    boxes = np.array([[-30.0, 0.0, 30.0, 60.0], [-1e4, -1e4, 1e4, 1e4]], dtype=np.float32)
    for x, y in zip(pa.query_aabb(boxes), pb.query_aabb(boxes)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    bodies = np.arange(1, 8, dtype=np.int32)
    for x, y in zip(pa.contacts(bodies), pb.contacts(bodies)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


# ---- 5. size ---------------------------------------------------------------------------------------------------------------------------
def test_cfg2_world_explicit_defaults(built_lib):
    """The cfg 2 world (stack(1000, 200)) with every material set explicitly to {0.3, 0}: three steps byte for byte with an untouched
    twin device world."""
    sc = scenes.stack(1000, 200)
    pa, pb = _world(sc), _world(sc)
    pa.set_materials(_all(pa), 0.3, 0.0)
    cfg = _cfg("multiple_sloppy")
    for s in range(3):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "after step %d" % s)
