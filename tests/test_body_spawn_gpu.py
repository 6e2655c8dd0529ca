"""Spawning bodies between steps (phx_world_add_bodies) and the batch inverse masses (phx_world_set_inverse_masses) on the device,
held to their specification twins: a world A that spawns must equal, byte for byte, a world B with the same history that makes the
same bodies with AddBody (and set_body_inverse_mass) — right after the call and after every following step; and the oracle World,
given phxo_world_add_body at the same points, in lockstep.  A spawn keeps the solver's cached schedule and the broadphase's splitters."""
import ctypes as C
import time
import zlib

import numpy as np
import pytest

import phyx_amd
from phyx_amd import Configuration, scenes
from phyx_amd.api import pinned_inv_inertia
from helpers import oracle_world
from spawn_lockstep import compare, step

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
NAMES = ("bodies", "manifolds", "contact points", "joints")
MODES = {"single": phyx_amd.ISLAND_SINGLE, "multiple": phyx_amd.ISLAND_MULTIPLE, "single_sloppy": phyx_amd.ISLAND_SINGLE_SLOPPY,
         "multiple_sloppy": phyx_amd.ISLAND_MULTIPLE_SLOPPY}
SCENES = {"stack": lambda: scenes.stack(6, 30),
          "wall": lambda: scenes.wall(14, 12),
          "falling": lambda: scenes.falling(300, width=80.0, ymax=260.0),
          "piles": lambda: scenes.piles(3, 50, ymax=220.0)}


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


def _world_bytes(pw):
    return b"".join(x.tobytes() for x in pw.state())


def _add_body_loop(pw, spawn):
    """The specification: one AddBody per row."""
    return np.array([pw.AddBody((float(r[0]), float(r[1])), float(r[2]), (float(r[3]), float(r[4]))) for r in spawn], dtype=np.int64)


def _batch(kind, bodies, rng, k):
    """(k, 5) rows {px, py, angle, half_x, half_y}: on top of existing bodies (new pairs in the very next step), far away, or rotated."""
    rows = np.zeros((k, 5), dtype=np.float32)
    if kind == "overlap":
        at = rng.choice(len(bodies), size=k, replace=False)
        rows[:, 0] = bodies["pos"]["x"][at] + rng.uniform(-3.0, 3.0, k).astype(np.float32)
        rows[:, 1] = bodies["pos"]["y"][at] + rng.uniform(-3.0, 3.0, k).astype(np.float32)
        rows[:, 3:5] = rng.uniform(2.0, 6.0, (k, 2)).astype(np.float32)
    elif kind == "far":
        rows[:, 0] = 20000.0 + 40.0 * np.arange(k, dtype=np.float32)
        rows[:, 1] = 9000.0
        rows[:, 3:5] = 5.0
    else:
        rows[:, 0] = rng.uniform(-60.0, 60.0, k).astype(np.float32)
        rows[:, 1] = rng.uniform(350.0, 500.0, k).astype(np.float32)
        rows[:, 2] = rng.uniform(-3.2, 3.2, k).astype(np.float32)
        rows[:, 3:5] = rng.uniform(1.0, 8.0, (k, 2)).astype(np.float32)
    return rows


@pytest.mark.parametrize("kind", ["overlap", "far", "rotated"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("scene", list(SCENES))
def test_spawn_equals_the_add_body_path(built_lib, scene, mode, kind):
    cfg = _cfg(MODES[mode])
    pa, pb = _world(SCENES[scene]()), _world(SCENES[scene]())
    for _ in range(20):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
    rng = np.random.default_rng(zlib.crc32(("%s/%s/%s" % (scene, mode, kind)).encode()))
    rows = _batch(kind, pa.bodies, rng, 40)
    n = pa.counts()[0]
    got = pa.add_bodies(rows)
    assert got.tolist() == list(range(n, n + len(rows)))
    assert _add_body_loop(pb, rows).tolist() == got.tolist()
    _same(pa, pb, "right after the spawn")
    for s in range(5):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "after step %d" % s)
    if kind == "overlap":
        m = pa.manifolds
        assert ((m["body1"] >= n) | (m["body2"] >= n)).any(), "the spawned bodies never touched anything"


def test_lockstep_with_the_oracle_world(oracle, built_lib):
    """A row spawned every 8 steps onto a stack, 60 steps: every byte compared with the oracle World after every step, the oracle's
    solver replaying the device's schedule; the oracle grows through its own AddBody (phxo_world_add_body)."""
    sc = scenes.stack(4, 12)
    cfg = _cfg(phyx_amd.ISLAND_MULTIPLE_SLOPPY)
    pw, ow = _world(sc), oracle_world(sc)
    assert pw.bodies.tobytes() == ow.bodies().tobytes()
    spawned = 0
    for s in range(60):
        if s and s % 8 == 0:
            rows = np.array([[-40.0 + 16.0 * k + 0.5 * (s % 3), 260.0, 0.1 * (k - 3), 5.0, 4.0] for k in range(6)], dtype=np.float32)
            idx = pw.add_bodies(rows)
            for r in rows:
                ow.add_body(float(r[0]), float(r[1]), float(r[2]), float(r[3]), float(r[4]))
            assert pw.body_states(idx.astype(np.int32)).tobytes() == ow.bodies()[idx].tobytes()
            spawned += len(rows)
        step(oracle, pw, ow, cfg, DT)
        compare(pw, ow, s)
    assert spawned == 42 and len(ow.joints()) > 0
    m = ow.manifolds()
    assert ((m["body1"] >= len(sc["px"])) | (m["body2"] >= len(sc["px"]))).any(), "no spawned body came to rest on the stack"


def _settled(gravity=0.0):
    """A gravity-free stack stepped until its schedule is reused (recoloured == 0 three steps running)."""
    cfg = _cfg(phyx_amd.ISLAND_SINGLE)
    pw = _world(scenes.stack(6, 10), gravity)
    seen = []
    for _ in range(60):
        pw.Update(DT, cfg)
        seen.append(pw.solver.stats().recoloured)
        if len(seen) >= 3 and seen[-3:] == [0, 0, 0]:
            break
    assert seen[-3:] == [0, 0, 0], seen
    return pw, cfg


def test_spawn_keeps_the_cached_schedule(built_lib):
    """Isolated bodies spawned far away before each of 10 steps: the schedule stays cached (recoloured == 0), the builds equal those of
    a twin without spawns, and the stack's bodies come out the same."""
    pa, cfg = _settled()
    pc, _ = _settled()
    n = pa.counts()[0]
    c0 = (pa.build_counts(), pc.build_counts())
    for s in range(10):
        rows = np.array([[30000.0 + 50.0 * (10 * s + k), -5000.0 + 30.0 * s, 0.2 * k, 5.0, 5.0] for k in range(10)], dtype=np.float32)
        pa.add_bodies(rows)
        pa.Update(DT, cfg)
        pc.Update(DT, cfg)
        assert pa.solver.stats().recoloured == 0, "step %d rebuilt the schedule" % s
        assert pc.solver.stats().recoloured == 0
    assert [x - y for x, y in zip(pa.build_counts(), c0[0])] == [x - y for x, y in zip(pc.build_counts(), c0[1])]
    a, c = pa.state(), pc.state()
    assert a[0][:n].tobytes() == c[0].tobytes()
    for name, x, y in zip(NAMES[1:], a[1:], c[1:]):
        assert x.tobytes() == y.tobytes(), name
    assert pa.counts()[0] == n + 100


def test_spawn_after_removal_and_growth(built_lib):
    """remove_outside / spawn cycles against an AddBody twin doing the same; one batch crosses the body buffers' capacity, one comes
    right after a removal (the removal's spare buffers, now the world's, are the ones that grow)."""
    cfg = _cfg(phyx_amd.ISLAND_MULTIPLE)
    sc = scenes.falling(200, width=80.0, ymax=200.0)
    pa, pb = _world(sc), _world(sc)
    box = (-120.0, -5.0, 120.0, 2000.0)
    rng = np.random.default_rng(11)
    for cycle in range(6):
        for _ in range(4):
            pa.Update(DT, cfg)
            pb.Update(DT, cfg)
            _same(pa, pb, "cycle %d" % cycle)
        ra, _ = pa.remove_outside(box)
        rb, _ = pb.remove_outside(box)
        assert ra == rb
        n = pa.counts()[0]
        k = 2 * n + 200 if cycle == 2 else 25 + 10 * cycle        # (cycle 2: past any capacity the buffers can have, 2 n + 64)
        rows = np.zeros((k, 5), dtype=np.float32)
        rows[:, 0] = rng.uniform(-100.0, 100.0, k)
        rows[:, 1] = 300.0 + 12.0 * np.arange(k) / 8.0 + rng.uniform(0.0, 2.0, k)
        rows[:, 2] = rng.uniform(-1.0, 1.0, k)
        rows[:, 3:5] = rng.uniform(2.0, 5.0, (k, 2))
        pa.add_bodies(rows)
        _add_body_loop(pb, rows)
        _same(pa, pb, "right after the spawn of cycle %d" % cycle)
        if cycle == 4:                                             # a removal right behind a spawn, then a spawn right behind that
            pa.remove_outside((-90.0, -5.0, 90.0, 2000.0))
            pb.remove_outside((-90.0, -5.0, 90.0, 2000.0))
            pa.add_bodies(rows[:7])
            _add_body_loop(pb, rows[:7])
            _same(pa, pb, "after remove + spawn in cycle %d" % cycle)
    for s in range(3):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "at the end, step %d" % s)


def test_spawned_bodies_are_first_class_at_once(built_lib):
    """Before the next step, the edits and the gathers work on the new indices, as on the twin's AddBody bodies."""
    cfg = _cfg(phyx_amd.ISLAND_SINGLE_SLOPPY)
    pa, pb = _world(scenes.stack(5, 20)), _world(scenes.stack(5, 20))
    for _ in range(10):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
    rows = np.array([[-30.0 + 15.0 * k, 320.0, 0.3 * k, 4.0, 6.0] for k in range(5)], dtype=np.float32)
    idx = pa.add_bodies(rows).astype(np.int32)
    assert _add_body_loop(pb, rows).tolist() == idx.tolist()
    for w in (pa, pb):
        w.set_velocities(idx[:3], np.array([[10.0, -5.0, 0.5], [0.0, 30.0, -1.0], [-8.0, 0.0, 2.0]], dtype=np.float32))
        w.add_accelerations(idx[1:4], np.array([[100.0, 0.0, 1.0], [0.0, -50.0, 0.0], [5.0, 5.0, 5.0]], dtype=np.float32))
        w.set_poses(idx[4:], np.array([[60.0, 280.0, 0.7]], dtype=np.float32))
    assert pa.body_states(idx).tobytes() == pb.body_states(idx).tobytes()
    assert pa.poses().tobytes() == pb.poses().tobytes()
    n = pa.counts()[0]
    buf = phyx_amd.api.DeviceBuffer(16 * n)
    try:
        pa.poses_device(buf.ptr.value)
        pa.sync()
        assert buf.to_host().tobytes() == pb.poses().tobytes()
    finally:
        buf.free()
    _same(pa, pb, "after the edits")
    for s in range(4):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "after step %d" % s)


def test_set_inverse_masses(built_lib):
    """Static (0, 0) and pinned (0, I) on old and spawned bodies, against a twin that uses set_body_inverse_mass; the next step rebuilds
    the schedule on both."""
    cfg = _cfg(phyx_amd.ISLAND_MULTIPLE)
    pa, pb = _world(scenes.stack(4, 15)), _world(scenes.stack(4, 15))
    for _ in range(10):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
    rows = np.array([[-20.0 + 12.0 * k, 250.0, 0.0, 5.0, 5.0] for k in range(4)], dtype=np.float32)
    new = pa.add_bodies(rows).astype(np.int32)
    _add_body_loop(pb, rows)
    for _ in range(2):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
    bodies = np.array([3, 17, new[0], new[2]], dtype=np.int32)
    values = np.array([[0.0, 0.0], [0.0, pinned_inv_inertia(5.0, 5.0)], [0.0, 0.0], [0.0, pinned_inv_inertia(5.0, 5.0)]], dtype=np.float32)
    pa.set_inverse_masses(bodies, values)
    for b, v in zip(bodies, values):
        pb.set_inverse_mass(int(b), float(v[0]), float(v[1]))
    _same(pa, pb, "right after set_inverse_masses")
    pa.set_inverse_masses([], np.zeros((0, 2), dtype=np.float32))           # an empty batch: nothing
    for s in range(6):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        if s == 0:
            assert pa.solver.stats().recoloured != 0 and pb.solver.stats().recoloured != 0
        _same(pa, pb, "after step %d" % s)
    b = pa.bodies
    assert (b["inv_mass"][bodies] == 0).all() and (b["inv_inertia"][bodies[::2]] == 0).all()


def test_rejections_leave_the_world_unchanged(built_lib):
    L = built_lib
    INVALID, STATE = phyx_amd.api._lib.PHX_ERR_INVALID, phyx_amd.api._lib.PHX_ERR_STATE
    cfg = _cfg(phyx_amd.ISLAND_SINGLE, 10)
    pw, twin = _world(scenes.stack(3, 10)), _world(scenes.stack(3, 10))
    for _ in range(2):
        pw.Update(DT, cfg)
        twin.Update(DT, cfg)
    n = pw.counts()[0]
    before = _world_bytes(pw)
    first = C.c_int32(-7)
    ok = np.array([[0.0, 300.0, 0.0, 5.0, 5.0]], dtype=np.float32)
    for bad in ([np.nan, 0.0, 0.0, 1.0, 1.0], [0.0, np.inf, 0.0, 1.0, 1.0], [0.0, 0.0, -np.inf, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 1.0],
                [0.0, 0.0, 0.0, 1.0, -2.0], [0.0, 0.0, 0.0, np.nan, 1.0]):
        rows = np.concatenate([ok, np.array([bad], dtype=np.float32)])          # (a valid row first: nothing of it may stay)
        assert L.phx_world_add_bodies(pw.h, rows.ctypes.data_as(C.c_void_p), len(rows), C.byref(first)) == INVALID
    assert L.phx_world_add_bodies(pw.h, ok.ctypes.data_as(C.c_void_p), -1, C.byref(first)) == INVALID
    assert L.phx_world_add_bodies(pw.h, None, 1, C.byref(first)) == INVALID
    assert first.value == -7
    vals = np.array([[0.0, 0.0], [1.0, 1.0]], dtype=np.float32)
    for idx in ([2, n], [-1, 3], [4, 4]):
        ix = np.array(idx, dtype=np.int32)
        assert L.phx_world_set_inverse_masses(pw.h, ix.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), 2) == INVALID
    ix = np.array([2, 3], dtype=np.int32)
    for v in ([[0.0, 0.0], [-1.0, 1.0]], [[0.0, -0.5], [1.0, 1.0]], [[np.nan, 0.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, np.inf]]):
        vv = np.array(v, dtype=np.float32)
        assert L.phx_world_set_inverse_masses(pw.h, ix.ctypes.data_as(C.c_void_p), vv.ctypes.data_as(C.c_void_p), 2) == INVALID
    assert L.phx_world_set_inverse_masses(pw.h, ix.ctypes.data_as(C.c_void_p), None, 2) == INVALID
    assert L.phx_world_set_inverse_masses(pw.h, None, vals.ctypes.data_as(C.c_void_p), 2) == INVALID
    assert L.phx_world_set_inverse_masses(pw.h, ix.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), -1) == INVALID
    assert _world_bytes(pw) == before
    # an empty call is a true no-op
    assert L.phx_world_add_bodies(pw.h, None, 0, C.byref(first)) == 0 and first.value == n
    # between PreSolve and FinishStep both are refused, and the world is unchanged by the attempt
    pw.PreSolve(DT)
    twin.PreSolve(DT)
    mid = _world_bytes(pw)
    for call in (lambda: pw.add_bodies(ok), lambda: pw.set_inverse_masses([1], np.zeros((1, 2), dtype=np.float32))):
        with pytest.raises(phyx_amd.PhxError) as e:
            call()
        assert e.value.status == STATE
    assert _world_bytes(pw) == mid
    pw.FinishStep(DT, cfg)
    twin.FinishStep(DT, cfg)
    for s in range(3):
        pw.Update(DT, cfg)
        twin.Update(DT, cfg)
        _same(pw, twin, "after step %d" % s)
    # a sharded world may not spawn (replica mode keeps the edit rules for set_inverse_masses)
    ps = _world(scenes.stack(3, 10))
    ps.set_shard(0, 2)
    shard_before = _world_bytes(ps)
    with pytest.raises(phyx_amd.PhxError) as e:
        ps.add_bodies(ok)
    assert e.value.status == STATE
    assert _world_bytes(ps) == shard_before


def test_cfg2_world(built_lib):
    """The cfg 2 world (stack(1000, 200), 200 001 bodies) 30 steps in: 2 000 bodies spawned above the stack, three steps against the
    AddBody twin."""
    t0 = time.perf_counter()
    cfg = _cfg(phyx_amd.ISLAND_SINGLE_SLOPPY, 20)
    sc = scenes.stack(1000, 200)
    pa, pb = _world(sc), _world(sc)
    for _ in range(30):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
    k = 2000
    rows = np.zeros((k, 5), dtype=np.float32)
    rows[:, 0] = (np.arange(k, dtype=np.float32) - k // 2) * 7.5
    rows[:, 1] = 2040.0 + 30.0 * (np.arange(k) % 3)
    rows[:, 2] = 0.01 * (np.arange(k) % 11)
    rows[:, 3:5] = 3.0
    idx = pa.add_bodies(rows)
    assert idx[0] == len(sc["px"])
    _add_body_loop(pb, rows)
    _same(pa, pb, "right after the spawn")
    for s in range(3):
        pa.Update(DT, cfg)
        pb.Update(DT, cfg)
        _same(pa, pb, "after step %d" % s)
    print("cfg 2 spawn test: %.1f s" % (time.perf_counter() - t0))


def test_emitter_example_runs(tmp_path, built_lib):
    """examples/emitter.c: rows spawned onto a static shelf and removed below a kill plane, from plain C, to the end."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "emitter")
    lib_dir = os.path.join(root, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "emitter.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    r = subprocess.run([exe, "300", "10", "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "481 bodies spawned" in r.stdout
    removed = int(r.stdout.split("bodies spawned, ")[1].split()[0])
    assert removed > 0, r.stdout
