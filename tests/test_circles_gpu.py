"""Round bodies on the device (phx_world_set_shapes; include/phyx_amd.h SHAPES), held to tests/circle_spec.py:
  - lockstep at the pre_solve boundary: every manifold's contact points after UpdateManifolds equal the spec's update of the previous
    step's slots on the bodies at the start of the step, byte for byte, in a pile where all three pair kinds occur in both body orders;
  - behaviour: a circle rolls down a slope a box rests on; two stacked circles come to rest;
  - twins: an active column of boxes against a world that never heard of shapes; set_state + set_shapes; save / load / fork / export;
  - plumbing: removal, spawn, add_circles; every rejection leaves the world unchanged; a resized box's AABB;
  - queries on both paths against the spec and against each other; the directed corpus (tests/query_corpus.py) on both paths, byte-equal
    to the spec and held to the float64 judge (tests/query_reference.py)."""
import ctypes as C

import numpy as np
import pytest

import circle_spec as spec
import phyx_amd
import query_corpus as qc
import shape_query_spec as sqs
from phyx_amd import Configuration, PhxError, SHAPE_BOX, SHAPE_CIRCLE, scenes
from phyx_amd.api import contact_point_dtype, manifold_dtype, rigid_body_dtype

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)
NAMES = ("bodies", "manifolds", "contact points", "joints")
F = np.float32


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _same(a, b, what):
    assert a.counts() == b.counts(), "counts differ %s" % what
    for name, x, y in zip(NAMES, a.state(), b.state()):
        assert x.tobytes() == y.tobytes(), "%s differ %s" % (name, what)


def _all(w):
    return np.arange(w.counts()[0], dtype=np.int32)


# The pile of the lockstep test: a ground box, then circles (radii 4 and 6) and boxes (half size 5) alternating in index order, so that a
# circle meets boxes with lower and with higher indices; two rows, each body overlapping its neighbours and the row below a little.
ROUND = {1: 4.0, 3: 6.0, 5: 4.0, 8: 6.0, 10: 4.0, 12: 6.0}      # body -> radius; the other bodies of 1 .. 12 are boxes


def mixed_world(extra_static_circle=False):
    w = phyx_amd.World(0, gravity=G)
    w.AddBody((0.0, 0.0), 0.0, (120.0, 10.0), static=True)
    row1 = [(-27.0, 1), (-18.5, 2), (-8.0, 3), (1.5, 4), (10.5, 5), (19.5, 6)]            # (x, body)
    row2 = [(-23.0, 7), (-13.0, 8), (-2.5, 9), (6.0, 10), (15.5, 11), (26.5, 12)]
    at = {}
    for x, b in row1:
        at[b] = (x, 10.0 + ROUND.get(b, 5.0) - 0.4)
    for x, b in row2:
        at[b] = (x, 10.0 + 9.0 + ROUND.get(b, 5.0) - 0.2)
    for b in range(1, 13):
        s = ROUND.get(b, 5.0)
        assert w.AddBody(at[b], 0.1 * b, (s, s)) == b
    idx = np.array(sorted(ROUND), dtype=np.int32)
    radii = np.array([ROUND[int(b)] for b in idx], dtype=np.float32)
    w.set_shapes(idx, SHAPE_CIRCLE, radii)
    w.set_inverse_masses(idx, phyx_amd.circle_inverse_masses(radii))
    if extra_static_circle:
        first = w.add_circles(np.array([[300.0, 300.0, 0.0, 5.0]], dtype=np.float32))
        w.set_inverse_masses([first], np.zeros((1, 2), dtype=np.float32))
    return w


def _kinds(w):
    return w.shapes()["kind"].astype(np.int32)


def _debug_update(lib, b1, b2, count, pts):
    r1, r2 = np.array([b1], dtype=rigid_body_dtype), np.array([b2], dtype=rigid_body_dtype)
    m = np.zeros(1, dtype=manifold_dtype)
    m["point_count"] = count
    p = np.array(pts, dtype=contact_point_dtype).copy()
    assert lib.phx_debug_update_manifold(_ptr(r1), 0, _ptr(r2), 0, _ptr(m), _ptr(p)) == 0
    return int(m["point_count"][0]), p


def _overlapping(bodies):
    """The unordered body pairs whose AABBs overlap (closed), by brute force; pairs of two static bodies left out."""
    lo = np.stack([bodies["aabb_min"]["x"], bodies["aabb_min"]["y"]], axis=1)
    hi = np.stack([bodies["aabb_max"]["x"], bodies["aabb_max"]["y"]], axis=1)
    static = (bodies["inv_mass"] == 0) & (bodies["inv_inertia"] == 0)
    out = set()
    for i in range(len(bodies)):
        for j in range(i + 1, len(bodies)):
            if static[i] and static[j]:
                continue
            if lo[i, 0] <= hi[j, 0] and hi[i, 0] >= lo[j, 0] and lo[i, 1] <= hi[j, 1] and hi[i, 1] >= lo[j, 1]:
                out.add((i, j))
    return out


# ---- 1. lockstep at the pre_solve boundary ------------------------------------------------------------------------------------------------
def test_update_manifolds_lockstep(built_lib):
    w = mixed_world()
    kinds = _kinds(w)
    assert kinds.tolist() == [1 if b in ROUND else 0 for b in range(13)]
    prev = {}                                               # (body1, body2) -> (point_count, its two slots) after the previous step
    seen = set()                                            # (kind1, kind2) of the manifolds that had a point
    blank = np.zeros(2, dtype=contact_point_dtype)
    blank["solver_index"] = -1
    for s in range(30):
        bodies = w.bodies
        w.PreSolve(DT)
        m, cp = w.manifolds, w.contactPoints
        now, live = {}, set()
        for k in range(len(m)):
            b1, b2 = int(m["body1"][k]), int(m["body2"][k])
            count, slots = prev.get((b1, b2), (0, blank))
            if kinds[b1] or kinds[b2]:
                want_n, want = spec.update_manifold(bodies[b1], kinds[b1], bodies[b2], kinds[b2], count, slots)
            else:
                want_n, want = _debug_update(built_lib, bodies[b1], bodies[b2], count, slots)
            got_n = int(m["point_count"][k])
            got = cp[m["point_index"][k]:m["point_index"][k] + 2].copy()
            assert got_n == want_n, "step %d, pair (%d, %d): %d points, the spec has %d" % (s, b1, b2, got_n, want_n)
            a, b = got[:got_n].copy(), want[:want_n].copy()
            a["solver_index"], b["solver_index"] = 0, 0                          # (the joint match's, not UpdateManifolds')
            assert a.tobytes() == b.tobytes(), "step %d, pair (%d, %d): %s != %s" % (s, b1, b2, a, b)
            now[(b1, b2)] = (got_n, got)
            live.add((min(b1, b2), max(b1, b2)))
            if got_n:
                seen.add((int(kinds[b1]), int(kinds[b2])))
        assert len(live) == len(m), "a pair has two manifolds"
        kept = {(min(a, b), max(a, b)) for (a, b), (n, _) in now.items() if (a, b) in prev and n > 0}
        assert live == _overlapping(bodies) | kept, "step %d: the manifold set is not the overlapping pairs and the live old ones" % s
        prev = now
        w.FinishStep(DT, CFG)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}, "pair kinds with points: %s" % sorted(seen)


# ---- 2. behaviour -----------------------------------------------------------------------------------------------------------------------
def test_a_circle_rolls_where_a_box_rests():
    """A 0.2 rad slope (tan 0.2 = 0.203 < 0.3, the default friction): the box stays, the circle rolls downhill and spins up."""
    w = phyx_amd.World(0, gravity=G)
    angle = 0.2
    w.AddBody((0.0, 0.0), angle, (300.0, 5.0), static=True)
    ground = w.bodies[0]
    xv = np.array([ground["xv"]["x"], ground["xv"]["y"]], dtype=np.float64)
    yv = np.array([ground["yv"]["x"], ground["yv"]["y"]], dtype=np.float64)
    on_slope = lambda s, size: tuple(s * xv + (5.0 + size - 0.05) * yv)      # noqa: E731
    box = w.AddBody(on_slope(80.0, 5.0), angle, (5.0, 5.0))
    circle = w.add_circles(np.array([[*on_slope(-40.0, 5.0), angle, 5.0]], dtype=np.float32))
    assert w.shapes()["kind"].tolist() == [0, 0, 1]
    start = w.bodies.copy()
    spins = []
    for s in range(90):
        w.Update(DT, CFG)
        if s in (29, 59, 89):
            spins.append(abs(float(w.bodies["angular_velocity"][circle])))
    end = w.bodies
    along = lambda b: float((end["pos"]["x"][b] - start["pos"]["x"][b]) * xv[0] + (end["pos"]["y"][b] - start["pos"]["y"][b]) * xv[1])      # noqa: E731
    print("box moved %.4f along the slope, the circle %.3f; |angular velocity| %s" % (along(box), along(circle), spins))
    assert abs(along(box)) < 0.5 and abs(float(end["angular_velocity"][box])) < 0.05
    assert along(circle) < -5.0, "the circle did not move downhill"
    assert spins[0] > 0.2 and spins[0] < spins[1] < spins[2], "the circle's angular velocity does not grow"


def test_two_stacked_circles_come_to_rest():
    w = phyx_amd.World(0, gravity=G)
    w.AddBody((0.0, 0.0), 0.0, (100.0, 10.0), static=True)
    first = w.add_circles(np.array([[0.0, 16.2, 0.3, 6.0], [0.0, 26.4, -0.2, 4.0]], dtype=np.float32))
    assert first == 1
    for _ in range(150):
        w.Update(DT, CFG)
    b = w.bodies
    y1, y2 = float(b["pos"]["y"][1]), float(b["pos"]["y"][2])
    pen_ground, pen_pair = 10.0 + 6.0 - y1, 6.0 + 4.0 - float(np.hypot(b["pos"]["x"][2] - b["pos"]["x"][1], y2 - y1))
    speed = float(np.abs(np.stack([b["velocity"]["x"][1:], b["velocity"]["y"][1:]])).max())
    print("penetration: ground %.4f, pair %.4f; largest velocity component %.4f" % (pen_ground, pen_pair, speed))
    assert -0.1 < pen_ground < 2.0 and -0.1 < pen_pair < 2.0, "the solver's displacement threshold is 2 units"
    # at rest the solver cancels what gravity adds in a step, |G| * DT = 3.3: a third of that is the bound on what is left
    assert speed < abs(G) * DT / 3.0 and abs(float(b["pos"]["x"][2])) < 0.5
    m = w.manifolds
    assert len(m) == 2 and (m["point_count"] == 1).all()


# ---- 3. twins -----------------------------------------------------------------------------------------------------------------------------
def test_active_column_of_boxes_steps_like_no_column():
    sc = scenes.stack(8, 8)
    a, b = phyx_amd.World(0, gravity=G), phyx_amd.World(0, gravity=G)
    a.add_scene(sc)
    b.add_scene(sc)
    size = b.bodies["geom_size"][5]
    b.set_shapes([5], SHAPE_CIRCLE, float(size["x"]))                           # the column exists from here on ...
    b.set_shapes([5], SHAPE_BOX, float(size["x"]), float(size["y"]))            # ... and every body is a box again
    assert (b.shapes()["kind"] == 0).all()
    for s in range(20):
        if s == 7:                                                               # once more on the device, after steps
            b.set_shapes([9], SHAPE_CIRCLE, float(size["x"]))
            b.set_shapes([9], SHAPE_BOX, float(size["x"]), float(size["y"]))
        a.Update(DT, CFG)
        b.Update(DT, CFG)
        _same(a, b, "after step %d" % s)
    assert b.shapes().tobytes() == a.shapes().tobytes()


def test_set_state_then_set_shapes_reproduces_a_circle_world():
    a = mixed_world()
    for _ in range(10):
        a.Update(DT, CFG)
    sh = a.shapes()
    b = phyx_amd.World(0, gravity=G)
    b.set_state(*a.state())
    assert (b.shapes()["kind"] == 0).all(), "set_state resets every kind to box"
    assert b.shapes()["hx"].tobytes() == sh["hx"].tobytes(), "the sizes are in the records"
    b.set_shapes(_all(b), sh["kind"], sh["hx"], sh["hy"])
    assert b.shapes().tobytes() == sh.tobytes()
    _same(a, b, "after set_state + set_shapes")
    for s in range(10):
        a.Update(DT, CFG)
        b.Update(DT, CFG)
        _same(a, b, "step %d after the restore" % s)


def test_snapshots_carry_the_kinds():
    a = mixed_world()
    for _ in range(6):
        a.Update(DT, CFG)
    snap = a.save()
    with pytest.raises(PhxError, match="circles"):
        snap.to_bytes()
    b = phyx_amd.World(0, gravity=G)
    b.load(snap)
    c = a.fork()
    for w in (b, c):
        assert w.shapes().tobytes() == a.shapes().tobytes()
        _same(a, w, "after the load")
    for s in range(8):
        for w in (a, b, c):
            w.Update(DT, CFG)
        _same(a, b, "step %d after the load" % s)
        _same(a, c, "step %d after the fork" % s)
    # a world loaded from a snapshot without the column has none
    plain = phyx_amd.World(0, gravity=G)
    plain.add_scene(scenes.stack(2, 3))
    b.load(plain.save())
    assert (b.shapes()["kind"] == 0).all() and b.counts()[0] == plain.counts()[0]
    # every body a box again: the blob carries the world
    sh = a.shapes()
    a.set_shapes(_all(a), SHAPE_BOX, sh["hx"], sh["hy"])
    a.save(snap)
    blob = snap.to_bytes()
    d = phyx_amd.World(0, gravity=G)
    d.load(phyx_amd.Snapshot.from_bytes(blob))
    assert (d.shapes()["kind"] == 0).all()
    _same(a, d, "after the blob")


# ---- 4. plumbing --------------------------------------------------------------------------------------------------------------------------
def test_removal_spawn_and_add_circles_move_the_kinds():
    w = mixed_world()
    for _ in range(4):
        w.Update(DT, CFG)
    kinds = _kinds(w)
    gone = [2, 3, 10]
    keep = np.ones(len(kinds), dtype=bool)
    keep[gone] = False
    before = w.shapes()
    remap = w.remove_bodies(gone)
    assert (remap[gone] == -1).all()
    kinds = spec.remove(kinds, keep)
    assert _kinds(w).tolist() == kinds.tolist()
    assert w.shapes().tobytes() == before[keep].tobytes()
    w.add_bodies(np.array([[60.0, 40.0, 0.0, 3.0, 2.0], [70.0, 40.0, 0.0, 2.0, 2.0]], dtype=np.float32))
    kinds = spec.spawn(kinds, 2)
    assert _kinds(w).tolist() == kinds.tolist()
    n = w.counts()[0]
    first = w.add_circles(np.array([[80.0, 40.0, 0.5, 3.0], [90.0, 40.0, 0.0, 7.0]], dtype=np.float32))
    assert first == n and w.counts()[0] == n + 2
    sh = w.shapes()
    assert sh["kind"].tolist() == kinds.tolist() + [1, 1] and sh["hx"][n:].tolist() == [3.0, 7.0] and sh["hy"][n:].tolist() == [3.0, 7.0]
    b = w.bodies
    for k, r in ((n, 3.0), (n + 1, 7.0)):
        im, ii = spec.circle_masses(r)
        assert b["inv_mass"][k] == im and b["inv_inertia"][k] == ii
    w.Update(DT, CFG)
    assert _kinds(w).tolist() == kinds.tolist() + [1, 1]
    # before the first step (host-staged bodies) the same calls act on the host's table
    h = phyx_amd.World(0, gravity=G)
    h.AddBody((0.0, 0.0), 0.0, (50.0, 5.0), static=True)
    assert h.add_circles(np.array([[0.0, 12.0, 0.0, 4.0]], dtype=np.float32)) == 1
    h.AddBody((20.0, 12.0), 0.0, (3.0, 3.0))
    assert h.shapes()["kind"].tolist() == [0, 1, 0]
    h.Update(DT, CFG)
    assert h.shapes()["kind"].tolist() == [0, 1, 0]


def test_rejections_leave_the_world_unchanged():
    w = mixed_world()
    for _ in range(3):
        w.Update(DT, CFG)
    state, sh = w.state(), w.shapes()

    def unchanged(what):
        assert w.shapes().tobytes() == sh.tobytes(), what
        for name, x, y in zip(NAMES, state, w.state()):
            assert x.tobytes() == y.tobytes(), "%s changed by %s" % (name, what)

    bad = {"a bad kind": ([2], 2, 3.0, 3.0), "a negative kind": ([2], -1, 3.0, 3.0), "hy != hx for a circle": ([2], SHAPE_CIRCLE, 3.0, 4.0),
           "an infinite size": ([2], SHAPE_BOX, np.inf, 3.0), "a NaN size": ([2], SHAPE_CIRCLE, np.nan, np.nan),
           "a zero size": ([2], SHAPE_BOX, 3.0, 0.0), "a negative size": ([2], SHAPE_CIRCLE, -3.0, -3.0),
           "a repeated index": ([2, 4, 2], SHAPE_BOX, 3.0, 3.0), "an index out of range": ([2, 13], SHAPE_BOX, 3.0, 3.0),
           "a bad entry behind good ones": ([2, 4], [0, 1], [3.0, 3.0], [3.0, 2.0])}
    for what, (idx, kind, hx, hy) in bad.items():
        with pytest.raises(PhxError) as e:
            w.set_shapes(idx, kind, hx, hy)
        assert e.value.status == phyx_amd._lib.PHX_ERR_INVALID, what
        unchanged(what)
    assert w.L.phx_world_set_shapes(w.h, None, None, 1) == phyx_amd._lib.PHX_ERR_INVALID
    assert w.L.phx_world_set_shapes(w.h, None, None, -1) == phyx_amd._lib.PHX_ERR_INVALID
    assert w.L.phx_world_set_shapes(w.h, None, None, 0) == 0
    unchanged("an empty call")
    w.PreSolve(DT)
    with pytest.raises(PhxError) as e:
        w.set_shapes([2], SHAPE_BOX, 3.0, 3.0)
    assert e.value.status == phyx_amd._lib.PHX_ERR_STATE
    w.FinishStep(DT, CFG)
    # sharded worlds carry no circles, and a world with a circle cannot be sharded
    with pytest.raises(PhxError) as e:
        w.set_shard(0, 2)
    assert e.value.status == phyx_amd._lib.PHX_ERR_STATE and "circles" in str(e.value)
    s = phyx_amd.World(0, gravity=G)
    s.add_scene(scenes.stack(2, 2))
    s.set_shard(0, 2)
    with pytest.raises(PhxError) as e:
        s.set_shapes([1], SHAPE_BOX, 3.0, 3.0)
    assert e.value.status == phyx_amd._lib.PHX_ERR_STATE


def _aabb(pos, xv, yv, size):
    """Geom::RecomputeAABB in float32 (ref: Geom.h:79-85), one operation at a time."""
    dx = np.abs(F(xv[0])) * F(size[0]) + np.abs(F(yv[0])) * F(size[1])
    dy = np.abs(F(xv[1])) * F(size[0]) + np.abs(F(yv[1])) * F(size[1])
    return [F(pos[0]) - dx, F(pos[1]) - dy, F(pos[0]) + dx, F(pos[1]) + dy]


@pytest.mark.parametrize("when", ["host_staged", "after_steps"])
def test_a_resized_box_gets_the_aabb_of_set_poses(when):
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scenes.stack(2, 3))
    if when == "after_steps":
        for _ in range(3):
            w.Update(DT, CFG)
    before = w.bodies
    w.set_shapes([2, 4], SHAPE_BOX, [7.0, 1.5], [2.0, 6.0])
    after = w.bodies
    for b, size in ((2, (7.0, 2.0)), (4, (1.5, 6.0))):
        r = after[b]
        assert (float(r["geom_size"]["x"]), float(r["geom_size"]["y"])) == size
        want = _aabb((r["pos"]["x"], r["pos"]["y"]), (r["xv"]["x"], r["xv"]["y"]), (r["yv"]["x"], r["yv"]["y"]), size)
        assert [r["aabb_min"]["x"], r["aabb_min"]["y"], r["aabb_max"]["x"], r["aabb_max"]["y"]] == want
        assert r["inv_mass"] == before[b]["inv_mass"] and r["inv_inertia"] == before[b]["inv_inertia"], "the masses are not touched"
    untouched = [k for k in range(len(after)) if k not in (2, 4)]
    assert after[untouched].tobytes() == before[untouched].tobytes()
    # set_poses of the same pose computes the same AABB from the new size
    poses = np.stack([[after[b]["pos"]["x"], after[b]["pos"]["y"], after[b]["xv"]["x"], after[b]["xv"]["y"], after[b]["yv"]["x"], after[b]["yv"]["y"]] for b in (2, 4)])
    w.set_poses([2, 4], poses.astype(np.float32))
    assert w.bodies.tobytes() == after.tobytes()
    assert (w.shapes()["kind"] == 0).all()
    w.Update(DT, CFG)
    assert w.shapes()["hx"][[2, 4]].tolist() == [7.0, 1.5]


# ---- 5. queries on both paths -------------------------------------------------------------------------------------------------------------
def _query_world(monkeypatch, path):
    monkeypatch.setenv("PHX_QUERY_PATH", path)
    w = mixed_world(extra_static_circle=True)
    for _ in range(5):
        w.Update(DT, CFG)
    return w


def _queries(bodies, kinds):
    rng = np.random.default_rng(5)
    pts = [rng.uniform((-40.0, 5.0), (40.0, 45.0), (150, 2))]
    rays = []
    for b in np.flatnonzero(kinds == 1):
        c, r = np.array([bodies["pos"]["x"][b], bodies["pos"]["y"][b]], dtype=np.float64), float(bodies["geom_size"]["x"][b])
        pts.append(np.array([c, c + 0.9 * r, c - 0.9 * r, c + (0.999 * r, 0.0), c + (1.001 * r, 0.0), c + (0.0, -r)]))
        for dx, dy in ((1.0, 0.0), (0.0, -1.0), (0.6, -0.8), (-1.0, 0.3)):
            d = np.array([dx, dy])
            rays.append([*(c - 60.0 * d), dx, dy, 200.0])                       # through the centre
            rays.append([*(c - 60.0 * d + 0.98 * r * np.array([-dy, dx])), dx, dy, 200.0])      # a grazing chord
            rays.append([*(c - 60.0 * d + 1.02 * r * np.array([-dy, dx])), dx, dy, 200.0])      # just past the rim
        rays.append([*c, 1.0, 0.0, 50.0])                                     # from inside
        rays.append([*(c + (1.5, 1.5 * r)), 1.0, -1.0, 200.0])                 # across the frame square's corner, past the disc
    rays += [[x, 80.0, 0.1, -1.0, 100.0] for x in np.linspace(-40.0, 40.0, 33)]
    rays += [[-80.0, y, 1.0, 0.02, 30.0] for y in np.linspace(8.0, 45.0, 9)]     # max_t short of most of the pile
    return np.concatenate(pts).astype(np.float32), np.array(rays, dtype=np.float32)


def test_queries_see_the_disc_on_both_paths(monkeypatch):
    got = {}
    for path in ("scan", "index"):
        w = _query_world(monkeypatch, path)
        bodies, kinds = w.bodies, _kinds(w)
        lone = len(bodies) - 1
        assert kinds[lone] == 1 and bodies["pos"]["x"][lone] == 300.0
        pts, rays = _queries(bodies, kinds)
        p, r = w.query_points(pts), w.raycast(rays)
        assert p.tobytes() == spec.query_points(bodies, kinds, pts).tobytes(), path
        want = spec.raycast(bodies, kinds, rays)
        assert r.tobytes() == want.tobytes(), "%s: %s" % (path, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(r, want)]))
        assert p.tobytes() != sqs_points(bodies, pts).tobytes(), "no point tells the disc from its frame square"
        # the lone static circle at (300, 300), r = 5: inside the frame square and outside the disc; a ray across the square's corner
        assert w.query_points([[304.5, 304.5], [303.0, 303.0]]).tolist() == [-1, lone]
        assert w.raycast([[301.5, 307.5, 1.0, -1.0, 100.0]])["body"].tolist() == [-1]
        assert w.raycast([[280.0, 300.0, 1.0, 0.0, 100.0]])["t"].tolist() == [15.0]
        assert w.query_points([[303.0, 303.0]], skip_static=True).tolist() == [-1]
        # oriented boxes and casts see the frame square
        boxes = np.array([[304.6, 304.6, 1.0, 0.0, 0.0, 1.0, 0.3, 0.3], [306.0, 306.0, 1.0, 0.0, 0.0, 1.0, 0.3, 0.3]] +
                         [phyx_amd.box_from_angle(x, 24.0, 0.3, 3.0, 2.0) for x in np.linspace(-30.0, 30.0, 9)], dtype=np.float32)
        off, hits = w.query_boxes(boxes)
        woff, whits = sqs.query_boxes(bodies, boxes)
        assert off.tobytes() == woff.tobytes() and hits.tobytes() == whits.tobytes(), path
        assert hits[off[0]:off[1]].tolist() == [lone] and off[2] == off[1]
        casts = np.array([[304.6, 320.0, 1.0, 0.0, 0.0, 1.0, 0.3, 0.3, 0.0, -1.0, 100.0]] +
                         [[x, 70.0, 1.0, 0.0, 0.0, 1.0, 2.0, 2.0, 0.0, -1.0, 100.0] for x in np.linspace(-30.0, 30.0, 9)], dtype=np.float32)
        c = w.cast_boxes(casts)
        assert c.tobytes() == sqs.cast_boxes(bodies, casts).tobytes(), path
        assert c["body"][0] == lone and abs(float(c["t"][0]) - 14.7) < 1e-4, "the cast stops at the frame square's top, y = 305"
        got[path] = (bodies.tobytes(), p.tobytes(), r.tobytes(), hits.tobytes(), c.tobytes())
    assert got["scan"] == got["index"]


def sqs_points(bodies, pts):
    import query_spec
    return query_spec.query_points(bodies, pts)


# ---- 6. the directed corpus on both paths: the spec's bytes, and the judge's bounds on the device's own answers ------------------------------
@pytest.mark.parametrize("path", ("scan", "index"))
@pytest.mark.parametrize("name", [c.name for c in qc.cases()])
def test_corpus_queries_equal_the_spec_and_meet_the_judge(monkeypatch, name, path):
    """A world built from the corpus case's bodies (no step): raycast and query_points are byte-equal to circle_spec, and the device's
    own answers meet the float64 judge by the bounds and the excused set of test_circles_cpu.test_spec_queries_against_the_float64_judge
    (a kernel that drifted from the spec would still be held to the truth).  "a row of discs from 3000" is the closest-hit choice
    among several discs seen from far away; "65 bodies" is one body past a tree node."""
    monkeypatch.setenv("PHX_QUERY_PATH", path)
    c = qc.case(name)
    w = qc.world(c.bodies, c.kinds)
    bodies, kinds = w.bodies, _kinds(w)
    assert kinds.tolist() == c.kinds.tolist()
    for rays in (c.rays, c.near_rays):
        if not len(rays):
            continue
        got, want = w.raycast(rays), spec.raycast(bodies, kinds, rays)
        assert got.tobytes() == want.tobytes(), "%s %s: rays %s" % (name, path, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[:8])
        _, worst = qc.judged("rays", qc.judge_hits, bodies, kinds, rays, got)
        if rays is c.rays:
            print("%s %s: worst in u: %s" % (name, path, qc.table(worst)))
            qc.assert_bounds(worst, "%s %s" % (name, path))
    for pts in (c.points, c.near_points):
        if not len(pts):
            continue
        got = w.query_points(pts)
        assert got.tobytes() == spec.query_points(bodies, kinds, pts).tobytes(), "%s %s: points" % (name, path)
        qc.judged("points", qc.judge_points, bodies, kinds, pts, got)
    if name == "a row of discs from 3000":
        assert w.raycast(c.rays)["body"].tolist() == [3, 2, -1, 3, 2, -1, 3, 2, -1, 1, 2, -1]
