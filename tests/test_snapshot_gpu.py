"""Device snapshots (include/phyx_amd.h SNAPSHOTS): save, load, fork and export a whole world.  "The same world" means byte-equal
bodies, manifolds, contact points, joints, the three column getters, the counts and the output of contact_events."""
import numpy as np
import pytest

import phyx_amd
import snapshot_cases as cases
import snapshot_spec as spec
from phyx_amd import BODY_SENSOR, Configuration, PhxError, Snapshot, World, scenes
from phyx_amd._lib import PHX_ERR_INVALID, PHX_ERR_STATE

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)
# falling(300) as the scene generator makes it, the same 300 boxes dropped close together (they overlap from the first step on:
# manifolds are born and die in every step), and the 22-body stack
SCENES = {"falling": lambda: scenes.falling(300),
          "falling_dense": lambda: scenes.falling(300, width=80.0, ymax=260.0),
          "stack": lambda: scenes.stack(3, 7)}


def _world(scene, gravity=G):
    w = World(0, gravity=gravity)
    w.add_scene(scene)
    return w


def _step(w, k=1):
    for _ in range(k):
        w.Update(DT, CFG)


def _state(w):
    b, m, c, j = w.state()
    return {"counts": w.counts(), "bodies": b.tobytes(), "manifolds": m.tobytes(), "contact points": c.tobytes(), "joints": j.tobytes(),
            "filters": w.collision_filters().tobytes(), "materials": w.materials().tobytes(), "flags": w.body_flags().tobytes()}


def _observe(w):
    """The state and what contact_events reports (which advances the baseline: both worlds of a comparison are observed alike)."""
    s = _state(w)
    begin, end = w.contact_events()
    s["begin"], s["end"] = begin.tobytes(), end.tobytes()
    return s


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], "%s: %s differ" % (what, k)


def _steps(w, k):
    out = []
    for _ in range(k):
        w.Update(DT, CFG)
        out.append(_observe(w))
    return out


def _same_steps(a, b, what=""):
    assert len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        _same(x, y, "%s step %d" % (what, s))


def _set_columns(w):
    """filters on 5 bodies, materials on 7, one sensor"""
    w.set_collision_filters([3, 4, 5, 6, 7], category=[2, 2, 4, 4, 1], mask=[0xFFFFFFFD, 0xFFFFFFFF, 0xFFFFFFFB, 3, 0xFFFFFFFF], group=[0, 0, 0, -1, -1])
    w.set_materials([1, 2, 3, 8, 9, 10, 11], friction=[0.0, 0.1, 0.9, 0.3, 2.0, 0.5, 0.05], restitution=[0.0, 0.5, 1.0, 0.25, 0.0, 0.75, 0.1])
    w.set_body_flags([12], BODY_SENSOR)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_rewind(built_lib, name):
    """Step 12, save, step 8 recording every step, load, step 8 again: every step is the same world as in the first pass, and the
    first step after the load rebuilds the solver's schedule."""
    w = _world(SCENES[name]())
    _step(w, 12)
    snap = w.save()
    assert snap.counts == w.counts()
    first = _steps(w, 8)
    w.load(snap)
    w.Update(DT, CFG)
    if w.counts()[3]:                                                       # (a step without joints builds no schedule)
        # 1 or 2: phx_solve_stats documents both as "the schedule was rebuilt" (2: without a host round trip, which a solver that has
        # built before may choose); a fresh world's first build is pinned to 1 in test_load_equals_the_old_path
        assert w.solver.stats().recoloured in (1, 2)
    again = [_observe(w)] + _steps(w, 7)
    _same_steps(first, again, name)
    if name != "falling":
        assert first[-1]["counts"][3] > 0


@pytest.mark.parametrize("name", ["falling", "falling_dense"])
def test_load_equals_the_old_path(built_lib, name):
    """A snapshot loaded into a fresh world, against a fresh world restored the documented old way — four getters, set_state, the three
    setters, saved right after a contact_events call: the same world for 6 steps."""
    w = _world(SCENES[name]())
    _set_columns(w)
    _step(w, 20)
    w.contact_events()                                                      # (the old path can only restore B = T(state))
    snap = w.save()
    a = World(0, gravity=G)
    a.load(snap)
    b = World(0, gravity=G)
    b.set_state(*w.state())
    n = w.counts()[0]
    f, mt, fl = w.collision_filters(), w.materials(), w.body_flags()
    assert b.set_collision_filters(np.arange(n), f["category"], f["mask"], f["group"]) == 0
    b.set_materials(np.arange(n), mt["friction"], mt["restitution"])
    b.set_body_flags(np.arange(n), fl)
    _same(_state(a), _state(b), "restored")
    _same(_state(a), _state(w), "against the saved world")
    a.Update(DT, CFG); b.Update(DT, CFG)
    if a.counts()[3]:
        assert a.solver.stats().recoloured == 1 and b.solver.stats().recoloured == 1      # (both rebuild the schedule)
    sa, sb, sw = [_observe(a)] + _steps(a, 5), [_observe(b)] + _steps(b, 5), _steps(w, 6)
    _same_steps(sa, sb, "load vs set_state")
    _same_steps(sa, sw, "load vs the saved world")
    if name == "falling_dense":
        assert sa[-1]["counts"][3] > 0


def test_columns_come_back(built_lib):
    w = _world(SCENES["falling_dense"]())
    _set_columns(w)
    _step(w, 10)
    snap = w.save()
    saved = _state(w)
    first = _steps(w, 4)
    w.set_collision_filters([3, 4, 20], category=[1, 8, 8], mask=[0xFFFFFFFF, 8, 8], group=[0, 0, 5])      # (body 3 back to the default)
    w.set_materials([1, 2, 30], friction=[0.3, 0.7, 0.0], restitution=[0.0, 0.0, 1.0])                       # (body 1 back to the default)
    w.set_body_flags([12, 13], [0, BODY_SENSOR])                                                             # (body 12 back to the default)
    _step(w, 2)
    w.load(snap)
    _same(_state(w), saved, "after the load")
    _same_steps(first, _steps(w, 4), "after the load")


def test_inactive_columns_load_as_defaults(built_lib):
    """A snapshot of a world that never set a column, loaded into a world with all three active: defaults for every body, and it steps
    bit for bit like a world that never heard of them."""
    plain, twin = _world(SCENES["falling_dense"]()), _world(SCENES["falling_dense"]())
    _step(plain, 10); _step(twin, 10)
    snap = plain.save()
    x = _world(SCENES["stack"]())
    _set_columns(x)
    _step(x, 3)
    x.load(snap)
    n = x.counts()[0]
    f = x.collision_filters()
    assert (f["category"] == 1).all() and (f["mask"] == 0xFFFFFFFF).all() and (f["group"] == 0).all()
    mt = x.materials()
    assert (mt["friction"] == np.float32(0.3)).all() and (mt["restitution"] == 0).all() and not x.body_flags().any() and n == 301
    _same_steps(_steps(twin, 4), _steps(x, 4), "defaults")


def test_counts_change(built_lib):
    w = _world(SCENES["stack"]())
    _step(w, 5)
    snap22 = w.save()
    first22 = _steps(w, 3)
    k = np.arange(300)
    spawn = np.stack([-600.0 + 12.0 * (k % 100), 200.0 + 12.0 * (k // 100), 0.1 * (k % 7), np.full(300, 4.0), np.full(300, 3.0)], axis=1).astype(np.float32)
    w.add_bodies(spawn)                                                     # (322 bodies: more than one workgroup, every body buffer grows)
    w.remove_bodies([2, 5, 9, 100, 321])
    _step(w, 3)
    w.load(snap22)
    assert w.counts()[0] == 22 and snap22.counts == w.counts()
    _same_steps(first22, _steps(w, 3), "back to 22 bodies")
    # the other direction: a 322-body snapshot into the 22-body world
    big = _world(SCENES["stack"]())
    _step(big, 5)
    big.add_bodies(spawn)
    _step(big, 2)
    snap322 = big.save()
    assert snap322.counts[0] == 322
    first322 = _steps(big, 3)
    w.load(snap22)
    w.load(snap322)
    assert w.counts()[0] == 322
    _same_steps(first322, _steps(w, 3), "up to 322 bodies")
    # no body, and one
    empty = World(0, gravity=G)
    w.load(empty.save())
    assert w.counts() == (0, 0, 0, 0)
    _step(w, 2)
    assert w.counts() == (0, 0, 0, 0) and len(w.bodies) == 0
    one = World(0, gravity=G)
    one.AddBody((0.0, 50.0), 0.3, (4.0, 2.0))
    w.load(one.save())
    assert w.counts() == (1, 0, 0, 0)
    _same_steps(_steps(one, 2), _steps(w, 2), "one body")


def test_baseline_is_restored_as_it_is(built_lib):
    """contact_events is NOT called before the save: B is empty while pairs touch, which set_state cannot restore."""
    w, twin = _world(SCENES["stack"]()), _world(SCENES["stack"]())
    _step(w, 4); _step(twin, 4)
    assert w.counts()[1] > 0
    snap = w.save()
    _step(w, 3)
    w.contact_events()                                                      # (advance B in between: the load must put the empty one back)
    w.load(snap)
    got, want = w.contact_events(), twin.contact_events()
    assert len(want[0]) > 0
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    _same_steps(_steps(twin, 2), _steps(w, 2), "after the events")


def test_pending_accelerations(built_lib):
    w = _world(SCENES["stack"]())
    _step(w, 3)
    w.add_accelerations([4, 9, 21], [[300.0, 0.0, 0.0], [0.0, 500.0, 2.0], [-100.0, 50.0, -1.0]])
    snap = w.save()
    saved = _state(w)
    first = _steps(w, 3)
    w.load(snap)
    _same(_state(w), saved, "pending accelerations in the records")
    _same_steps(first, _steps(w, 3), "pending accelerations")
    plain = _world(SCENES["stack"]())
    _step(plain, 4)
    assert _state(plain)["bodies"] != first[0]["bodies"], "the accelerations must have acted"


def test_host_staged(built_lib):
    """Save before the first step, and after set_inverse_mass following a step (which restages the bodies on the host)."""
    w, twin = _world(SCENES["stack"]()), _world(SCENES["stack"]())
    w.set_materials([3], friction=0.9)
    twin.set_materials([3], friction=0.9)
    snap = w.save()
    _step(w, 3)
    w.load(snap)
    _same(_state(w), _state(twin), "before the first step")
    _same_steps(_steps(twin, 3), _steps(w, 3), "from before the first step")
    for x in (w, twin):
        x.set_inverse_mass(5, 0.0, 0.0)
    snap = w.save()
    _step(w, 2)
    w.load(snap)
    _same(_state(w), _state(twin), "after set_inverse_mass")
    _same_steps(_steps(twin, 3), _steps(w, 3), "from the restaged world")


def test_fork(built_lib):
    """World A saves, world B loads, no synchronisation in between; saving A again while B's load is only queued does not disturb B."""
    a = _world(SCENES["falling_dense"]())
    _step(a, 10)
    snap = a.save()
    b = World(0, gravity=G)
    b.load(snap)
    _step(a, 1)
    a.save(snap)                                                            # (overwrites the snapshot B was loaded from)
    c = a.fork()
    a.load(snap)                                                            # (A is back where it saved last: one step ahead of B)
    a.contact_events(); c.contact_events()                                  # (B's first observation below advances its baseline to this step too)
    sb = _steps(b, 7)
    sa = _steps(a, 6)
    sc = _steps(c, 6)
    _same_steps(sb[1:], sa, "fork")
    _same_steps(sa, sc, "World.fork")
    assert c.gravity == a.gravity


@pytest.mark.parametrize("path", ["index", "scan"])
def test_queries_see_the_load(built_lib, monkeypatch, path):
    """PHX_QUERY_PATH is read when a world is created, so the environment of this process picks the path, as in tests/test_queries_gpu.py."""
    monkeypatch.setenv("PHX_QUERY_PATH", path)
    w = _world(SCENES["stack"]())
    _step(w, 2)
    old = w.bodies[7]
    at_old = np.array([[old["pos"]["x"], old["pos"]["y"]]], dtype=np.float32)
    at_new = np.array([[500.0, 700.0]], dtype=np.float32)
    assert w.query_points(at_old)[0] == 7 and w.query_points(at_new)[0] == -1
    snap = w.save()
    w.set_poses([7], [phyx_amd.api.frame_from_angle(500.0, 700.0, 0.0)])
    assert w.query_points(at_new)[0] == 7 and w.query_points(at_old)[0] != 7
    w.load(snap)
    assert w.query_points(at_old)[0] == 7 and w.query_points(at_new)[0] == -1


def test_blob_round_trip(built_lib):
    w = _world(SCENES["falling_dense"]())
    _set_columns(w)
    _step(w, 9)                                                             # (B stays empty while pairs touch: the blob carries it so)
    w.add_accelerations([6], [[10.0, 20.0, 0.5]])
    snap = w.save()
    blob = snap.to_bytes()
    b, m, c, j = w.state()
    assert blob == spec.pack(b, m, c, j, w.collision_filters(), w.materials(), w.body_flags(), baseline=np.zeros((0, 2), np.int32))
    assert spec.check(blob) is None
    other = Snapshot.from_bytes(blob)
    assert other.counts == snap.counts and other.to_bytes() == blob
    x, y = World(0, gravity=G), World(0, gravity=G)
    x.load(snap); y.load(other)
    _same(_state(x), _state(y), "loaded")
    _same_steps(_steps(x, 4), _steps(y, 4), "blob")
    # a blob with a baseline that is not empty
    w.contact_events()
    blob2 = w.save().to_bytes()
    assert blob2 == spec.pack(b, m, c, j, w.collision_filters(), w.materials(), w.body_flags()) and blob2 != blob
    # bad blobs: refused, the snapshot and the world as they were
    before = _state(y)
    for name in ("truncated_by_one", "joint_not_pointed_back", "restitution_1_5"):
        bad = cases.mutations()[name]
        assert built_lib.phx_snapshot_import(other.h, bad, len(bad)) == PHX_ERR_INVALID, name
        assert b"phx_snapshot_import" in built_lib.phx_last_error()
    assert other.to_bytes() == blob
    _same(_state(y), before, "after the refused imports")
    # the hand-made state through a blob into a world
    hb, hm, hc, hj = cases.state_three_bodies()
    z = World(0, gravity=G)
    z.load(Snapshot.from_bytes(cases.three_body_blob()))
    assert z.bodies.tobytes() == hb.tobytes() and z.contactJoints.tobytes() == hj.tobytes() and z.manifolds.tobytes() == hm.tobytes()
    assert z.materials().tobytes() == cases.columns(3)[1].tobytes() and z.collision_filters().tobytes() == cases.columns(3)[0].tobytes()
    assert z.body_flags().tolist() == [0, 1, 0]


def test_refusals(built_lib):
    w, twin = _world(SCENES["stack"]()), _world(SCENES["stack"]())
    _step(w, 3); _step(twin, 3)
    snap = w.save()
    L = built_lib
    # mid-step
    w.PreSolve(DT)
    assert L.phx_world_save(w.h, snap.h) == PHX_ERR_STATE and L.phx_world_load(w.h, snap.h) == PHX_ERR_STATE
    w.FinishStep(DT, CFG)
    _step(twin, 1)
    # an empty snapshot
    empty = Snapshot()
    assert L.phx_world_load(w.h, empty.h) == PHX_ERR_STATE
    with pytest.raises(PhxError):
        empty.counts
    with pytest.raises(PhxError):
        empty.to_bytes()
    # NULL handles
    assert L.phx_world_save(w.h, None) == PHX_ERR_INVALID and L.phx_world_load(None, snap.h) == PHX_ERR_INVALID
    # sharded
    w.set_shard(0, 2)
    assert L.phx_world_save(w.h, snap.h) == PHX_ERR_STATE and L.phx_world_load(w.h, snap.h) == PHX_ERR_STATE
    w.set_shard(0, 1)
    _same_steps(_steps(twin, 3), _steps(w, 3), "after the refusals")
    assert snap.counts[0] == 22


def test_wrong_device_is_refused(built_lib):
    if phyx_amd.device_count() < 2:
        pytest.skip("one device: a snapshot of another device cannot be made")
    w = _world(SCENES["stack"]())
    other = Snapshot(1)
    assert built_lib.phx_world_save(w.h, other.h) == PHX_ERR_INVALID
    assert built_lib.phx_world_load(w.h, other.h) == PHX_ERR_INVALID
