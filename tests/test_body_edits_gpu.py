"""Edits of body state between steps (phx_world_add_accelerations / set_velocities / set_poses) and the O(count) gathers
(phx_world_get_body_states / get_poses / get_poses_device), in lockstep with the oracle World given the same writes: the reference's
own demo loop (ref: main.cpp:337-349, the mouse drag on body 1) runs on the device, every byte compared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration, scenes
from phyx_amd.api import frame_from_angle
from helpers import oracle_world, oracle_set_pose as _oracle_set_pose, oracle_set_velocity as _oracle_set_velocity

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compare(pw, ow, step):
    assert pw.counts() == (len(ow.bodies()), len(ow.manifolds()), len(ow.contact_points()), len(ow.joints())), "step %d" % step
    assert pw.manifolds.tobytes() == ow.manifolds().tobytes(), "manifolds differ at step %d" % step
    assert pw.contactJoints.tobytes() == ow.joints().tobytes(), "joints differ at step %d" % step
    assert pw.bodies.tobytes() == ow.bodies().tobytes(), "bodies differ at step %d" % step
    m = ow.manifolds()
    first, count = m["point_index"].astype(np.int64), m["point_count"].astype(np.int64)
    live = np.repeat(first - (np.cumsum(count) - count), count) + np.arange(int(count.sum()), dtype=np.int64)
    assert pw.contactPoints[live].tobytes() == ow.contact_points()[live].tobytes(), "contact points differ at step %d" % step


def _step(oracle, pw, ow, cfg):
    """One World::Update on both sides, the oracle's solver replaying the device's schedule (test_world_gpu.py _lockstep)."""
    pw.Update(DT, cfg)
    ow.pre_solve(DT)
    order, offs = pw.solver.schedule()
    groups, _ = pw.solver.groups()
    b, cp, j = ow.bodies(), ow.contact_points(), ow.joints()
    assert len(order) == len(j)
    oracle.solver_solve_grouped(b, cp, j, order, offs, groups, cfg.contactIterationsCount, cfg.penetrationIterationsCount, oracle.STAG_COLOUR_SYNC)
    ow.integrate_position(DT)


def _lockstep(oracle, scene, steps, cfg, before_step=None, check_every=1, pw=None, ow=None):
    """Like test_world_gpu.py's _lockstep, with `before_step(pw, ow, step)` making the same writes on both worlds before each Update."""
    if pw is None:
        pw = phyx_amd.World(0, gravity=G)
        pw.add_scene(scene)
        ow = oracle_world(scene)
        assert pw.bodies.tobytes() == ow.bodies().tobytes()
    for step in range(steps):
        if before_step is not None:
            before_step(pw, ow, step)
        _step(oracle, pw, ow, cfg)
        if step % check_every == 0 or step == steps - 1:
            _compare(pw, ow, step)
    return pw, ow


def _oracle_add_accel(ow, i, a):
    b = ow.bodies()
    b["acceleration"]["x"][i] += a[0]
    b["acceleration"]["y"][i] += a[1]
    b["angular_acceleration"][i] += a[2]


def _oracle_frame(oracle, px, py, angle):
    """The frame the oracle's own RigidBody constructor gives a body at `angle` (an independent check of set_poses' angle form)."""
    rec = np.zeros(1, dtype=oracle.body_dtype)
    oracle.lib().phxo_body_init(C.c_void_p(rec.ctypes.data), px, py, angle, 1.0, 1.0, 1e-5)
    return np.array([px, py, rec["xv"]["x"][0], rec["xv"]["y"][0], rec["yv"]["x"][0], rec["yv"]["y"][0]], dtype=np.float32)


class Drag:
    """The demo's controller on body 1 (ref: main.cpp:337-346) toward a target moving along `waypoints` at `speed` units per step."""

    def __init__(self, waypoints, speed):
        self.points = [np.asarray(p, dtype=np.float64) for p in waypoints]
        self.speed = float(speed)
        self.contacts = 0

    def target(self, step):
        left = self.speed * step
        for a, b in zip(self.points, self.points[1:]):
            d = float(np.linalg.norm(b - a))
            if left <= d:
                return (a + (b - a) * (left / d)).astype(np.float32)
            left -= d
        return self.points[-1].astype(np.float32)

    def accel(self, state, step):
        pos = np.array([state["pos"]["x"][0], state["pos"]["y"][0]], dtype=np.float32)
        vel = np.array([state["velocity"]["x"][0], state["velocity"]["y"][0]], dtype=np.float32)
        dst = (self.target(step) - pos) * np.float32(50.0)
        a = np.array([0.0, -G], dtype=np.float32)
        a += (dst - vel) * np.float32(5.0)
        return np.array([a[0], a[1], 0.0], dtype=np.float32)

    def __call__(self, pw, ow, step):
        st = pw.body_states([1])
        assert st.tobytes() == ow.bodies()[1:2].tobytes(), "body 1 differs before step %d" % step
        a = self.accel(st, step)
        pw.add_accelerations([1], a[None, :])
        _oracle_add_accel(ow, 1, a)
        m = ow.manifolds()
        touching = ((m["body1"] == 1) & (m["body2"] > 1)) | ((m["body2"] == 1) & (m["body1"] > 1))
        self.contacts += int(touching.sum())


# the start of body 1 is (-1000, 1500) in every reference scene (ref: main.cpp:90-95)
DRAGS = {
    4: [(-1000.0, 1500.0), (-120.0, 500.0), (-120.0, 100.0), (150.0, 100.0)],          # down onto the tapered stacks, then through them
    7: [(-1000.0, 1500.0), (-200.0, 1650.0), (-200.0, 60.0), (-60.0, 60.0)],           # over the splitter at x = -300, into its boxes
}


@pytest.mark.parametrize("scene,island_mode", [(4, phyx_amd.ISLAND_SINGLE), (7, phyx_amd.ISLAND_MULTIPLE_SLOPPY)])
def test_demo_drag_lockstep(oracle, built_lib, scene, island_mode):
    drag = Drag(DRAGS[scene], 45.0)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, island_mode, 15, 15)
    _lockstep(oracle, scenes.reference(scene, boxes=360), 60, cfg, before_step=drag, check_every=3)
    assert drag.contacts > 0, "body 1 never touched the stack: the drag did not reach the solver"


def test_teleports_and_velocity_writes_mid_run(oracle, built_lib):
    scene = scenes.stack(6, 40)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)

    def edits(pw, ow, step):
        if step != 20:
            return
        m = ow.manifolds()
        in_contact = sorted(set(m["body1"][m["body1"] > 0].tolist()) | set(m["body2"][m["body2"] > 0].tolist()))
        moved = [in_contact[3], in_contact[40], in_contact[100]]
        b = ow.bodies()
        over = (float(b["pos"]["x"][150]) + 3.0, float(b["pos"]["y"][150]) + 2.0)      # body 7 lands half inside body 150
        frames = np.stack([frame_from_angle(300.0, 40.0, 0.0), frame_from_angle(-200.0, 300.0, 0.7)])
        pw.set_poses(moved[:2], frames)
        angles = np.array([[over[0], over[1], 0.4], [500.0, 25.0, -1.2]], dtype=np.float32)
        pw.set_poses([7, moved[2]], angles)
        for i, p in zip(moved[:2], frames):
            _oracle_set_pose(oracle, ow, i, p)
        for i, (x, y, a) in zip([7, moved[2]], angles):
            _oracle_set_pose(oracle, ow, i, _oracle_frame(oracle, float(x), float(y), float(a)))
        vel = np.array([[40.0, 300.0, 2.0], [-25.0, 0.0, -1.5], [0.0, -80.0, 0.0]], dtype=np.float32)
        pw.set_velocities([12, 60, 200], vel)
        for i, v in zip([12, 60, 200], vel):
            _oracle_set_velocity(ow, i, v)
        assert pw.body_states([7]).tobytes() == ow.bodies()[7:8].tobytes()

    pw, ow = _lockstep(oracle, scene, 45, cfg, before_step=edits, check_every=1)
    assert len(ow.joints()) > 0


def _poses_of(records):
    return np.stack([records["pos"]["x"], records["pos"]["y"], records["xv"]["x"], records["xv"]["y"]], axis=1).astype(np.float32)


def _check_gathers(pw, rng, k=64):
    b = pw.bodies
    idx = rng.integers(0, len(b), size=k).astype(np.int32)
    assert pw.body_states(idx).tobytes() == b[idx].tobytes()
    assert pw.poses().tobytes() == _poses_of(b).tobytes()
    buf = phyx_amd.api.DeviceBuffer(16 * len(b))
    try:
        pw.poses_device(buf.ptr.value)
        pw.sync()
        assert buf.to_host().tobytes() == _poses_of(b).tobytes()
    finally:
        buf.free()


@pytest.mark.parametrize("scene", ["small", "cfg2"])
def test_records_and_gathers(built_lib, scene):
    sc = scenes.stack(6, 40) if scene == "small" else scenes.stack(1000, 200)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 10, 10)
    rng = np.random.default_rng(7)
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(sc)
    _check_gathers(pw, rng)                                                  # host-staged, before the first step
    for _ in range(3):
        pw.Update(DT, cfg)
    _check_gathers(pw, rng)
    n = pw.counts()[0]
    a1 = np.array([[1.5, -2.0, 0.25], [3.0, 4.0, -1.0]], dtype=np.float32)
    a2 = np.array([[0.5, 7.0, 0.125]], dtype=np.float32)
    pw.add_accelerations([5, n - 1], a1)
    pw.add_accelerations([5], a2)                                            # a second call on the same body sums, in call order
    b = pw.bodies
    assert b["acceleration"]["x"][5] == np.float32(np.float32(0.0) + a1[0, 0]) + a2[0, 0]
    assert b["acceleration"]["y"][5] == np.float32(a1[0, 1]) + a2[0, 1]
    assert b["angular_acceleration"][5] == np.float32(a1[0, 2]) + a2[0, 2]
    assert (b["acceleration"]["x"][n - 1], b["acceleration"]["y"][n - 1], b["angular_acceleration"][n - 1]) == tuple(a1[1])
    assert np.count_nonzero(b["acceleration"]["x"]) == 2
    _check_gathers(pw, rng)
    pw.set_velocities([9, 10], np.array([[1.0, 2.0, 3.0], [-4.0, -5.0, -6.0]], dtype=np.float32))
    _check_gathers(pw, rng)
    assert pw.body_states([9, 10])["angular_velocity"].tolist() == [3.0, -6.0]
    pw.set_poses([11], np.array([[50.0, 600.0, 0.3]], dtype=np.float32))
    _check_gathers(pw, rng)
    assert pw.poses()[11].tolist() == frame_from_angle(50.0, 600.0, 0.3)[:4].tolist()
    pw.Update(DT, cfg)
    b = pw.bodies
    assert not b["acceleration"]["x"].any() and not b["acceleration"]["y"].any() and not b["angular_acceleration"].any()
    _check_gathers(pw, rng)


def test_edits_before_the_first_step_and_across_host_staging(oracle, built_lib):
    scene = scenes.stack(5, 20)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE, 15, 15)
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scene)
    ow = oracle_world(scene)
    # right after add_scene: the records are host-staged
    a = np.array([[30.0, 100.0, 0.5]], dtype=np.float32)
    pw.add_accelerations([3], a); _oracle_add_accel(ow, 3, a[0])
    v = np.array([[5.0, 0.0, -0.25]], dtype=np.float32)
    pw.set_velocities([4], v); _oracle_set_velocity(ow, 4, v[0])
    p = frame_from_angle(-90.0, 80.0, 0.2)
    pw.set_poses([6], p[None, :]); _oracle_set_pose(oracle, ow, 6, p)
    assert pw.bodies.tobytes() == ow.bodies().tobytes()
    _lockstep(oracle, scene, 5, cfg, pw=pw, ow=ow)

    # edits queued on the device, then host-staging calls before the next step: the download must keep them
    pw.add_accelerations([8, 9], np.array([[0.0, 400.0, 0.0], [-50.0, 0.0, 1.0]], dtype=np.float32))
    _oracle_add_accel(ow, 8, (0.0, 400.0, 0.0)); _oracle_add_accel(ow, 9, (-50.0, 0.0, 1.0))
    pw.set_velocities([10], np.array([[0.0, 150.0, 0.0]], dtype=np.float32)); _oracle_set_velocity(ow, 10, (0.0, 150.0, 0.0))
    p = frame_from_angle(60.0, 250.0, -0.4)
    pw.set_poses([11], p[None, :]); _oracle_set_pose(oracle, ow, 11, p)
    pw.set_inverse_mass(12, 0.0, 0.0)
    b = ow.bodies(); b["inv_mass"][12] = 0.0; b["inv_inertia"][12] = 0.0
    i = pw.AddBody((0.0, 400.0), 0.3, (6.0, 4.0))
    assert ow.add_body(0.0, 400.0, 0.3, 6.0, 4.0) == i
    # now host-staged again: edits go into the staged records, and add to the accelerations they carry
    pw.add_accelerations([8, i], np.array([[1.0, 2.0, 3.0], [0.0, 50.0, 0.0]], dtype=np.float32))
    _oracle_add_accel(ow, 8, (1.0, 2.0, 3.0)); _oracle_add_accel(ow, i, (0.0, 50.0, 0.0))
    assert pw.bodies.tobytes() == ow.bodies().tobytes()
    _lockstep(oracle, scene, 10, cfg, pw=pw, ow=ow)


def _world_bytes(pw):
    return b"".join(x.tobytes() for x in pw.state())


def test_rejections(built_lib):
    L = built_lib
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scenes.stack(3, 10))
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 10, 10)
    for _ in range(2):
        pw.Update(DT, cfg)
    n = pw.counts()[0]
    before = _world_bytes(pw)
    fns = [(L.phx_world_add_accelerations, 3), (L.phx_world_set_velocities, 3), (L.phx_world_set_poses, 6)]
    for fn, width in fns:
        for idx in ([2, n], [-1], [4, 5, 4]):                       # out of range (after a valid one), negative, a duplicate
            ix = np.array(idx, dtype=np.int32)
            vals = np.ones((len(ix), width), dtype=np.float32)
            assert fn(pw.h, ix.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), len(ix)) == phyx_amd.api._lib.PHX_ERR_INVALID
        ix = np.array([1], dtype=np.int32)
        vals = np.ones((1, width), dtype=np.float32)
        assert fn(pw.h, ix.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), -1) == phyx_amd.api._lib.PHX_ERR_INVALID
    out = np.zeros(2, dtype=phyx_amd.api.rigid_body_dtype)
    ix = np.array([0, n], dtype=np.int32)
    assert L.phx_world_get_body_states(pw.h, ix.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p)) == phyx_amd.api._lib.PHX_ERR_INVALID
    assert _world_bytes(pw) == before
    # between PreSolve and FinishStep every edit is refused, and the world is unchanged by the attempt
    pw.PreSolve(DT)
    mid = _world_bytes(pw)
    for call in (lambda: pw.add_accelerations([1], np.ones((1, 3), dtype=np.float32)),
                 lambda: pw.set_velocities([1], np.ones((1, 3), dtype=np.float32)),
                 lambda: pw.set_poses([1], frame_from_angle(0.0, 50.0, 0.0)[None, :])):
        with pytest.raises(phyx_amd.PhxError) as e:
            call()
        assert e.value.status == phyx_amd.api._lib.PHX_ERR_STATE
    assert _world_bytes(pw) == mid
    pw.FinishStep(DT, cfg)
    pw.add_accelerations([1], np.ones((1, 3), dtype=np.float32))         # between steps again
    assert pw.body_states([1])["acceleration"]["x"][0] == 1.0


def test_schedule_cache_untouched_by_edits(built_lib):
    """Velocity / pose / acceleration edits change no joint topology: ten steps with a drag on an isolated body rebuild and reuse
    the schedule exactly as ten steps without it, and the stack's bodies come out the same."""
    sc = scenes.stack(6, 40)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)

    def run(edit):
        pw = phyx_amd.World(0, gravity=G)
        pw.add_scene(sc)
        lone = pw.AddBody((5000.0, 600.0), 0.0, (5.0, 5.0))
        for _ in range(40):                                         # settle
            pw.Update(DT, cfg)
        counts0 = pw.build_counts()
        reuse = []
        for s in range(10):
            if edit:
                pw.add_accelerations([lone], np.array([[10.0 + s, -G, 0.5]], dtype=np.float32))
                pw.set_velocities([lone], np.array([[20.0, 0.0, 0.0]], dtype=np.float32))
            pw.Update(DT, cfg)
            st = pw.solver.stats()
            reuse.append((st.recoloured, st.graph_replay, st.colour_count, st.island_count))
        counts1 = pw.build_counts()
        b = pw.bodies
        return (counts1[0] - counts0[0], counts1[1] - counts0[1]), reuse, b[:lone].tobytes(), b[lone]

    plain = run(False)
    dragged = run(True)
    assert dragged[0] == plain[0] and dragged[1] == plain[1]
    assert dragged[2] == plain[2]
    assert dragged[3]["pos"]["x"] > plain[3]["pos"]["x"]                 # (the edits did act on the lone body)


def test_full_size_drag_lockstep(oracle, built_lib):
    """The cfg 2 world (stack(1000, 200), 200 001 bodies, the benchmark's configuration) with the drag on body 1, three steps."""
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 20, 20)
    sc = scenes.stack(1000, 200)
    drag = Drag([(0.0, 400.0), (0.0, 300.0)], 20.0)
    _lockstep(oracle, sc, 3, cfg, before_step=drag, check_every=1)


def test_drag_example_moves_body_1_toward_its_target(tmp_path, built_lib):
    """examples/drag.c: the demo loop from plain C through the C ABI."""
    exe = str(tmp_path / "drag")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "drag.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [s for s in r.stdout.splitlines() if s.startswith("body 1:")][0]
    f = line.replace(",", " ").replace("(", " ").replace(")", " ").split()
    start, end, target = (float(f[3]), float(f[4])), (float(f[6]), float(f[7])), (float(f[9]), float(f[10]))
    d0 = np.hypot(target[0] - start[0], target[1] - start[1])
    d1 = np.hypot(target[0] - end[0], target[1] - end[1])
    assert d1 < 0.1 * d0, line
    assert "world:" in r.stdout


def test_staging_regrown_under_queued_edits(built_lib):
    """Three edits queued back to back with no read in between, sized so that the second outgrows both the pinned staging buffer (made
    at its 64 KB floor by the first: 4096 * (4 + 24) B = 112 KB) and the batch's place on the device while the first copy and scatter
    may still be queued; the third is a bump allocation in the regrown buffer, or its reuse from offset 0.  Every value must arrive."""
    n, side = 4096, 64
    k = np.arange(n)
    spawn = np.stack([(k % side) * 10.0, (k // side) * 10.0, np.zeros(n), np.full(n, 2.0), np.full(n, 2.0)], axis=1).astype(np.float32)
    pw = phyx_amd.World(0, gravity=0.0)
    pw.add_bodies(spawn)
    pw.Update(DT, Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE_SLOPPY, 10, 10))      # the device copy is the world
    rng = np.random.default_rng(11)
    first, second = np.arange(100, 116, dtype=np.int32), np.arange(3000, 3016, dtype=np.int32)
    v1 = rng.uniform(-50.0, 50.0, size=(16, 3)).astype(np.float32)
    v2 = rng.uniform(-50.0, 50.0, size=(16, 3)).astype(np.float32)
    order = rng.permutation(n).astype(np.int32)
    angle = rng.uniform(-3.0, 3.0, size=n)
    poses = np.stack([rng.uniform(-1e4, 1e4, size=n), rng.uniform(-1e4, 1e4, size=n), np.cos(angle), np.sin(angle), -np.sin(angle), np.cos(angle)],
                     axis=1).astype(np.float32)
    pw.set_velocities(first, v1)
    pw.set_poses(order, poses)
    pw.set_velocities(second, v2)
    b = pw.bodies
    assert len(b) == n
    got_v = np.stack([b["velocity"]["x"], b["velocity"]["y"], b["angular_velocity"]], axis=1)
    assert got_v[first].tobytes() == v1.tobytes()
    assert got_v[second].tobytes() == v2.tobytes()
    got_p = np.stack([b["pos"]["x"], b["pos"]["y"], b["xv"]["x"], b["xv"]["y"], b["yv"]["x"], b["yv"]["y"]], axis=1)
    assert got_p[order].tobytes() == poses.tobytes()
    others = np.ones(n, dtype=bool)
    others[first] = False
    others[second] = False
    assert not got_v[others].any()                                           # (no gravity, no contact: the step left every velocity 0)
