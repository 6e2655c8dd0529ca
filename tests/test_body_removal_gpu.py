"""Removal of bodies between steps (phx_world_remove_bodies / phx_world_remove_outside) on the device, held to its specification
(tests/removal_spec.py): a world A that removes bodies must equal, byte for byte, a fresh world B given
set_state(filter(A's state before, R)) — right after the removal and after every one of the following steps, with the same
schedule on the first of them.  set_state itself is pinned to the reference's World::Update (tests/test_reference_gpu.py)."""
import ctypes as C
import time
import zlib

import numpy as np
import pytest

import phyx_amd
import removal_spec
from phyx_amd import Configuration, scenes
from phyx_amd.api import rigid_body_dtype

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


def _world(scene):
    pw = phyx_amd.World(0, gravity=G)
    pw.add_scene(scene)
    return pw


def _pair(scene, cfg, steps, add_body=False):
    """Two worlds stepped alike: A, which removes (its records stay stale: nothing reads them), and its copy, whose state() is
    A's state before the removal."""
    ws = [_world(scene) for _ in range(2)]
    for w in ws:
        for _ in range(steps):
            w.Update(DT, cfg)
        if add_body:
            w.AddBody((0.0, 400.0), 0.3, (6.0, 4.0))
    return ws


def _same(a, b, what):
    assert a.counts() == b.counts(), "counts differ %s" % what
    for name, x, y in zip(NAMES, a.state(), b.state()):
        assert x.tobytes() == y.tobytes(), "%s differ %s" % (name, what)


def _twin(pa, filtered, cfg, steps=5, before_step=None):
    """World B from set_state(filtered); A and B compared now and after each of `steps` steps (the schedule on the first)."""
    pb = phyx_amd.World(0, gravity=G)
    pb.set_state(*filtered)
    _same(pa, pb, "right after the removal")
    for s in range(steps):
        for w in (pa, pb):
            if before_step is not None:
                before_step(w, s)
            w.Update(DT, cfg)
        if s == 0 and pa.counts()[3]:
            (oa, ca), (ob, cb) = pa.solver.schedule(), pb.solver.schedule()
            assert oa.tobytes() == ob.tobytes() and ca.tobytes() == cb.tobytes(), "the first step's schedules differ"
            (ga, la), (gb, lb) = pa.solver.groups(), pb.solver.groups()
            assert ga.tobytes() == gb.tobytes() and la == lb, "the first step's groups differ"
        _same(pa, pb, "after step %d" % s)
    return pb


def _static(bodies):
    return np.flatnonzero((bodies["inv_mass"] == 0) & (bodies["inv_inertia"] == 0)).astype(np.int32)


CASES = ("after0", "after1", "after20", "add_body", "nothing", "everything", "ground")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("scene", list(SCENES))
def test_removal_equals_set_state_of_the_filtered_state(built_lib, scene, mode, case):
    cfg = _cfg(MODES[mode])
    steps = {"after0": 0, "after1": 1}.get(case, 20)
    pa, copy = _pair(SCENES[scene](), cfg, steps, add_body=case == "add_body")
    before = copy.state()
    n = len(before[0])
    rng = np.random.default_rng(zlib.crc32(("%s/%s/%s" % (scene, mode, case)).encode()))
    if case == "nothing":
        removed = np.zeros(0, dtype=np.int32)
    elif case == "everything":
        removed = rng.permutation(n).astype(np.int32)
    elif case == "ground":
        removed = _static(before[0])
        assert len(removed) >= 1
    else:
        removed = rng.choice(n, size=max(1, n // 10), replace=False).astype(np.int32)
        if case == "add_body":
            removed = np.unique(np.append(removed, [n - 1, 1])).astype(np.int32)      # the added body and a neighbour of the ground
    remap = pa.remove_bodies(removed)
    filtered, new = removal_spec.filter(before, removed)
    assert remap.tolist() == new.tolist()
    if case == "nothing":
        # a true no-op: A steps exactly like its untouched copy, and its cached schedule is still good for that
        for s in range(3):
            pa.Update(DT, cfg)
            copy.Update(DT, cfg)
            assert pa.solver.stats().recoloured == copy.solver.stats().recoloured, "step %d" % s
            _same(pa, copy, "after step %d" % s)
        return
    _twin(pa, filtered, cfg)
    if case == "everything":
        assert pa.counts() == (0, 0, 0, 0)


def test_empty_call_keeps_the_schedule_cached(built_lib):
    """remove_bodies([]) before every step: each step rebuilds the schedule exactly when the same step without the call does, and
    once the contacts stop changing (a stack without gravity: nothing moves) the steps reuse it (recoloured == 0) after the call too."""
    cfg = _cfg(phyx_amd.ISLAND_SINGLE)
    pa, copy = _world(scenes.stack(6, 10)), _world(scenes.stack(6, 10))
    for w in (pa, copy):
        w.gravity = 0.0
    counts = (pa.build_counts(), copy.build_counts())
    seen = []
    for s in range(60):
        assert pa.remove_bodies([]).tolist() == list(range(pa.counts()[0]))
        pa.Update(DT, cfg)
        copy.Update(DT, cfg)
        seen.append((pa.solver.stats().recoloured, copy.solver.stats().recoloured))
        assert seen[-1][0] == seen[-1][1], seen
        if len(seen) >= 3 and all(a == 0 for a, _ in seen[-3:]):
            break
    assert all(a == 0 for a, _ in seen[-3:]), seen
    assert [x - y for x, y in zip(pa.build_counts(), counts[0])] == [x - y for x, y in zip(copy.build_counts(), counts[1])]
    _same(pa, copy, "after the steps")


@pytest.mark.parametrize("mode", list(MODES))
def test_first_step_after_a_removal_replayed_by_the_oracle(oracle, built_lib, mode):
    """The solve of the first step after a removal, on the device's schedule, equals the oracle's solver on the device's inputs."""
    cfg = _cfg(MODES[mode])
    pa = _world(scenes.piles(3, 50, ymax=220.0))
    for _ in range(20):
        pa.Update(DT, cfg)
    n = pa.counts()[0]
    rng = np.random.default_rng(5)
    pa.remove_bodies(rng.choice(n, size=n // 10, replace=False))
    pa.PreSolve(DT)
    b, cp, j = pa.bodies, pa.contactPoints, pa.contactJoints
    assert len(j) > 0
    pa.FinishStep(DT, cfg)
    order, offs = pa.solver.schedule()
    groups, _ = pa.solver.groups()
    ob, oj = b.view(oracle.body_dtype).copy(), j.view(oracle.joint_dtype).copy()
    oracle.solver_solve_grouped(ob, cp.view(oracle.contact_point_dtype), oj, order, offs, groups, cfg.contactIterationsCount,
                                cfg.penetrationIterationsCount, oracle.STAG_COLOUR_SYNC)
    assert pa.contactJoints.tobytes() == oj.tobytes(), "impulses differ from the oracle's"
    got, want = pa.bodies, ob.view(rigid_body_dtype)
    assert got["velocity"].tobytes() == want["velocity"].tobytes() and got["angular_velocity"].tobytes() == want["angular_velocity"].tobytes()


def test_remove_outside_after_teleports(built_lib):
    """set_poses moves three bodies out of the box; remove_outside takes exactly those, as remove_bodies of them does."""
    cfg = _cfg(phyx_amd.ISLAND_MULTIPLE_SLOPPY)
    scene = scenes.stack(6, 30)
    pa, copy = _pair(scene, cfg, 20)
    pc = _pair(scene, cfg, 20)[0]
    box = (-200.0, -50.0, 200.0, 600.0)
    gone = [3, 50, 100]
    frames = np.stack([phyx_amd.api.frame_from_angle(x, y, 0.3) for x, y in [(900.0, 40.0), (0.0, 2000.0), (-700.0, -300.0)]])
    for w in (pa, copy, pc):
        w.set_poses(gone, frames)
    before = copy.state()
    assert removal_spec.outside(before[0], box).tolist() == gone
    removed, remap = pa.remove_outside(np.array(box))
    assert removed == 3
    assert remap.tolist() == pc.remove_bodies(gone).tolist()
    _same(pa, pc, "remove_outside against remove_bodies")
    filtered, new = removal_spec.filter(before, gone)
    assert remap.tolist() == new.tolist()
    _twin(pa, filtered, cfg)


def test_remove_outside_with_every_body_inside_is_a_no_op(built_lib):
    cfg = _cfg(phyx_amd.ISLAND_SINGLE)
    pa, copy = _pair(scenes.stack(6, 30), cfg, 20)
    removed, remap = pa.remove_outside((-1e5, -1e5, 1e5, 1e5))
    assert removed == 0 and remap.tolist() == list(range(pa.counts()[0]))
    for s in range(3):
        pa.Update(DT, cfg)
        copy.Update(DT, cfg)
        assert pa.solver.stats().recoloured == copy.solver.stats().recoloured
        _same(pa, copy, "after step %d" % s)


def test_drag_continues_on_the_remapped_index(built_lib):
    """The demo's dragged body 1 (ref: main.cpp:337-346) after the ground, the rest of its column and others went: its index is
    remap[1] now, and the drag lifts it."""
    cfg = _cfg(phyx_amd.ISLAND_MULTIPLE)
    pa, copy = _pair(scenes.stack(6, 30), cfg, 10)
    before = copy.state()
    removed = [0] + list(range(2, 31)) + [40, 41, 120]
    remap = pa.remove_bodies(removed)
    filtered, new = removal_spec.filter(before, removed)
    i = int(remap[1])
    assert i == 0 and new[1] == 0
    start = pa.body_states([i])[0]["pos"]["y"]

    def drag(w, s):
        w.add_accelerations([i], np.array([[0.0, 900.0, 0.5]], dtype=np.float32))

    _twin(pa, filtered, cfg, before_step=drag)
    assert pa.body_states([i])[0]["pos"]["y"] > start + 1.0, "the drag did not act on the remapped body"


def test_poses_device_after_a_removal(built_lib):
    cfg = _cfg(phyx_amd.ISLAND_SINGLE_SLOPPY)
    pa = _world(scenes.stack(6, 30))
    for _ in range(5):
        pa.Update(DT, cfg)
    n = pa.counts()[0]
    pa.remove_bodies(np.arange(0, n, 3))
    m = pa.counts()[0]
    assert m == n - len(range(0, n, 3))
    buf = phyx_amd.api.DeviceBuffer(16 * n)
    try:
        pa.poses_device(buf.ptr.value)
        pa.sync()
        got = buf.to_host(16 * m).view(np.float32).reshape(m, 4)
        b = pa.bodies
        want = np.stack([b["pos"]["x"], b["pos"]["y"], b["xv"]["x"], b["xv"]["y"]], axis=1).astype(np.float32)
        assert got.tobytes() == want.tobytes()
        assert pa.poses().tobytes() == want.tobytes()
        with pytest.raises(phyx_amd.PhxError):
            pa.poses_device(buf.ptr.value, cap=m - 1)
    finally:
        buf.free()


def _world_bytes(pw):
    return b"".join(x.tobytes() for x in pw.state())


def test_rejections_leave_the_world_unchanged(built_lib):
    L = built_lib
    INVALID, STATE = phyx_amd.api._lib.PHX_ERR_INVALID, phyx_amd.api._lib.PHX_ERR_STATE
    cfg = _cfg(phyx_amd.ISLAND_SINGLE, 10)
    pw = _world(scenes.stack(3, 10))
    for _ in range(2):
        pw.Update(DT, cfg)
    n = pw.counts()[0]
    before = _world_bytes(pw)
    remap = np.full(n, 77, dtype=np.int32)
    for idx in ([2, n], [-1], [4, 5, 4]):                           # out of range (after a valid one), negative, a duplicate
        ix = np.array(idx, dtype=np.int32)
        assert L.phx_world_remove_bodies(pw.h, ix.ctypes.data_as(C.c_void_p), len(ix), remap.ctypes.data_as(C.c_void_p)) == INVALID
    ix = np.array([1], dtype=np.int32)
    assert L.phx_world_remove_bodies(pw.h, ix.ctypes.data_as(C.c_void_p), -1, None) == INVALID
    removed = C.c_int32(-5)
    for box in ([0.0, 0.0, np.nan, 1.0], [0.0, 0.0, -1.0, 1.0], [0.0, 2.0, 1.0, 1.0], [-np.inf, 0.0, 1.0, 1.0]):
        b = np.array(box, dtype=np.float32)
        assert L.phx_world_remove_outside(pw.h, b.ctypes.data_as(C.c_void_p), C.byref(removed), remap.ctypes.data_as(C.c_void_p)) == INVALID
    assert L.phx_world_remove_outside(pw.h, None, C.byref(removed), None) == INVALID
    assert (remap == 77).all()
    assert _world_bytes(pw) == before
    # between PreSolve and FinishStep both are refused, and the world is unchanged by the attempt
    pw.PreSolve(DT)
    mid = _world_bytes(pw)
    for call in (lambda: pw.remove_bodies([1]), lambda: pw.remove_outside((-1.0, -1.0, 1.0, 1.0))):
        with pytest.raises(phyx_amd.PhxError) as e:
            call()
        assert e.value.status == STATE
    assert _world_bytes(pw) == mid
    pw.FinishStep(DT, cfg)
    # a sharded world is refused, as set_state refuses it
    ps = _world(scenes.stack(3, 10))
    ps.set_shard(0, 2)
    shard_before = _world_bytes(ps)
    for call in (lambda: ps.remove_bodies([1]), lambda: ps.remove_outside((-1.0, -1.0, 1.0, 1.0))):
        with pytest.raises(phyx_amd.PhxError) as e:
            call()
        assert e.value.status == STATE
    assert _world_bytes(ps) == shard_before
    # the handle is still good
    remap = pw.remove_bodies([1])
    assert remap[0] == 0 and remap[1] == -1 and remap[2] == 1 and pw.counts()[0] == n - 1
    pw.Update(DT, cfg)


def test_cfg2_world(built_lib):
    """The cfg 2 world (stack(1000, 200), 200 001 bodies) 30 steps in: 10 % random bodies, then a kill-plane box, against the twin."""
    t0 = time.perf_counter()
    cfg = _cfg(phyx_amd.ISLAND_SINGLE_SLOPPY, 20)
    pa, copy = _pair(scenes.stack(1000, 200), cfg, 30)
    before = copy.state()
    del copy
    n = len(before[0])
    rng = np.random.default_rng(2)
    r1 = rng.choice(n, size=n // 10, replace=False).astype(np.int32)
    remap1 = pa.remove_bodies(r1)
    mid, new1 = removal_spec.filter(before, r1)
    assert remap1.tolist() == new1.tolist()
    box = (-6000.0, -100.0, 6000.0, 1500.0)
    r2 = removal_spec.outside(mid[0], box)
    assert len(r2) > 10000
    removed, remap2 = pa.remove_outside(box)
    assert removed == len(r2)
    filtered, new2 = removal_spec.filter(mid, r2)
    assert remap2.tolist() == new2.tolist()
    _twin(pa, filtered, cfg, steps=3)
    print("cfg 2 removal test: %.1f s" % (time.perf_counter() - t0))
