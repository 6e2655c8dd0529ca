"""Capsule bodies on the device (phx_world_set_shapes with PHX_SHAPE_CAPSULE; include/phyx_amd.h SHAPES), held to tests/capsule_spec.py:
  - lockstep at the pre_solve boundary: every manifold's contact points after UpdateManifolds equal the spec's update of the previous
    step's slots on the bodies at the start of the step, byte for byte, in a pile where all nine pairs of kinds occur;
  - behaviour: a capsule rests on its side with two points, topples from its end, stays on a slope a circle rolls down; six logs pile up;
  - twins: a capsule named and taken back against a world that never heard of one; set_state + set_shapes; save / load / fork;
  - plumbing: removal, spawn, add_capsules; every rejection leaves the world unchanged;
  - queries on both paths against the spec, every part of a capsule winning."""
import numpy as np
import pytest

import capsule_spec as spec
import phyx_amd
import round_query_spec as rqs
import shape_query_spec as sqs
from phyx_amd import Configuration, DeviceBuffer, PhxError, SHAPE_BOX, SHAPE_CAPSULE, SHAPE_CIRCLE, scenes
from phyx_amd.api import contact_point_dtype, ray_hit_dtype, shape_hit_dtype
from test_circles_gpu import _debug_update, _overlapping, _same, _all, _kinds, mixed_world, NAMES

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)
F = np.float32

# The pile of the lockstep test: a ground box, a static capsule and a static circle just above it as rounded stops, then two rows in which
# boxes (half size 4), circles (radius 4) and capsules ({7, 4}) follow each other so that every kind meets every kind with the lower and
# with the higher index; each body overlaps its neighbours and the row below a little.
ROW1 = [2, 2, 0, 1, 1, 2, 1, 0]            # bodies 3 .. 10
ROW2 = [0, 1, 2, 0, 2, 2, 1]               # bodies 11 .. 17
HALF = {0: 4.0, 1: 4.0, 2: 7.0}


def _row(kinds, x0, y, overlap, first_angle):
    rows, x = [], x0
    for k, kind in enumerate(kinds):
        x += HALF[kind]
        rows.append((x, y, first_angle + 0.03 * k if kind == 2 else 0.1 * k, HALF[kind], 4.0, kind))
        x += HALF[kind] - overlap
    return rows


def capsule_world():
    w = phyx_amd.World(0, gravity=G)
    w.AddBody((0.0, 0.0), 0.0, (150.0, 10.0), static=True)
    w.AddBody((-58.5, 14.2), 0.0, (7.0, 4.0), static=True)                       # the stops at the ends of the lower row, clear of the ground:
    w.AddBody((30.0, 14.2), 0.0, (4.0, 4.0), static=True)                        # bodies 1 and 2, a capsule and a circle below
    w.set_shapes([1, 2], [SHAPE_CAPSULE, SHAPE_CIRCLE], [7.0, 4.0], [4.0, 4.0])
    rows = _row(ROW1, -52.0, 10.0 + 4.0 - 0.4, 0.5, -0.06)
    rows += _row(ROW2, -46.0, 10.0 + 8.0 + 4.0 - 0.6, 0.5, 0.05)
    a = np.array(rows, dtype=np.float64)
    idx = w.add_bodies(a[:, :5].astype(F))
    kinds = a[:, 5].astype(np.int32)
    for kind, masses in ((SHAPE_CIRCLE, lambda s: phyx_amd.circle_inverse_masses(s[:, 3])), (SHAPE_CAPSULE, lambda s: phyx_amd.capsule_inverse_masses(s[:, 3], s[:, 4]))):
        sel = np.flatnonzero(kinds == kind)
        w.set_shapes(idx[sel], kind, a[sel, 3].astype(F), a[sel, 4].astype(F))
        w.set_inverse_masses(idx[sel], masses(a[sel].astype(F)))
    return w


# ---- 1. lockstep at the pre_solve boundary ------------------------------------------------------------------------------------------------
def test_update_manifolds_lockstep(built_lib):
    w = capsule_world()
    kinds = _kinds(w)
    assert kinds.tolist() == [0, 2, 1] + ROW1 + ROW2
    prev, seen, two = {}, set(), set()
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
            assert got_n == want_n, "step %d, pair (%d, %d) of kinds (%d, %d): %d points, the spec has %d" % (s, b1, b2, kinds[b1], kinds[b2], got_n, want_n)
            a, b = got[:got_n].copy(), want[:want_n].copy()
            a["solver_index"], b["solver_index"] = 0, 0                          # (the joint match's, not UpdateManifolds')
            assert a.tobytes() == b.tobytes(), "step %d, pair (%d, %d): %s != %s" % (s, b1, b2, a, b)
            now[(b1, b2)] = (got_n, got)
            live.add((min(b1, b2), max(b1, b2)))
            if got_n:
                seen.add((int(kinds[b1]), int(kinds[b2])))
            if got_n == 2 and 2 in (kinds[b1], kinds[b2]):
                two.add((int(kinds[b1]), int(kinds[b2])))
        assert len(live) == len(m), "a pair has two manifolds"
        kept = {(min(a, b), max(a, b)) for (a, b), (n, _) in now.items() if (a, b) in prev and n > 0}
        assert live == _overlapping(bodies) | kept, "step %d: the manifold set is not the overlapping pairs and the live old ones" % s
        prev = now
        w.FinishStep(DT, CFG)
    print("pair kinds with points: %s; capsule pairs with two: %s" % (sorted(seen), sorted(two)))
    assert seen == {(a, b) for a in range(3) for b in range(3)}, "pair kinds with points: %s" % sorted(seen)
    assert two, "no capsule manifold had two points"


# ---- 2. behaviour -----------------------------------------------------------------------------------------------------------------------
def _angle(b, k):
    return float(np.arctan2(b["xv"]["y"][k], b["xv"]["x"][k]))


def _penetrations(w):
    """(p2 - p1) . n of every stored contact point."""
    b, m, cp = w.bodies, w.manifolds, w.contactPoints
    out = []
    for k in range(len(m)):
        for q in cp[m["point_index"][k]:m["point_index"][k] + m["point_count"][k]]:
            p1 = np.array([b["pos"]["x"][m["body1"][k]] + q["delta1"]["x"], b["pos"]["y"][m["body1"][k]] + q["delta1"]["y"]], dtype=np.float64)
            p2 = np.array([b["pos"]["x"][m["body2"][k]] + q["delta2"]["x"], b["pos"]["y"][m["body2"][k]] + q["delta2"]["y"]], dtype=np.float64)
            out.append(float((p2 - p1) @ np.array([q["normal"]["x"], q["normal"]["y"]], dtype=np.float64)))
    return np.array(out)


def test_a_capsule_rests_on_its_side_with_two_points():
    w = phyx_amd.World(0, gravity=G)
    w.AddBody((0.0, 0.0), 0.0, (100.0, 10.0), static=True)
    assert w.add_capsules(np.array([[0.0, 13.2, 0.02, 9.0, 3.0]], dtype=F)) == 1
    for _ in range(150):
        w.Update(DT, CFG)
    b, m = w.bodies, w.manifolds
    speed = float(np.abs([b["velocity"]["x"][1], b["velocity"]["y"][1]]).max())
    pen = 10.0 + 3.0 - float(b["pos"]["y"][1])
    print("angle %.5f, penetration %.4f, largest velocity component %.4f, points %s" % (_angle(b, 1), pen, speed, m["point_count"].tolist()))
    assert len(m) == 1 and m["point_count"].tolist() == [2]
    assert abs(_angle(b, 1)) < 0.02 and -0.1 < pen < 2.0
    # at rest the solver cancels what gravity adds in a step, |G| * DT = 3.3: a third of that is the bound on what is left
    assert speed < abs(G) * DT / 3.0 and abs(float(b["angular_velocity"][1])) < 0.05


def test_a_capsule_stood_on_end_topples():
    w = phyx_amd.World(0, gravity=G)
    w.AddBody((0.0, 0.0), 0.0, (200.0, 10.0), static=True)
    w.add_capsules(np.array([[0.0, 10.0 + 9.0 - 0.1, np.pi / 2 + 0.1, 9.0, 2.0]], dtype=F))
    w.Update(DT, CFG)
    assert w.manifolds["point_count"].tolist() == [1], "on its end a capsule has one point"
    for _ in range(299):
        w.Update(DT, CFG)
    b = w.bodies
    print("angle %.4f, height %.4f, points %s" % (_angle(b, 1), float(b["pos"]["y"][1]), w.manifolds["point_count"].tolist()))
    assert abs(np.sin(_angle(b, 1))) < 0.05, "the capsule does not lie on its side"
    assert abs(float(b["pos"]["y"][1]) - 12.0) < 2.0 and w.manifolds["point_count"].tolist() == [2]


def test_a_capsule_stays_where_a_circle_rolls():
    """A 0.2 rad slope (tan 0.2 = 0.203 < 0.3, the default friction): the capsule lying along it stays, the circle rolls downhill."""
    w = phyx_amd.World(0, gravity=G)
    angle = 0.2
    w.AddBody((0.0, 0.0), angle, (300.0, 5.0), static=True)
    ground = w.bodies[0]
    xv = np.array([ground["xv"]["x"], ground["xv"]["y"]], dtype=np.float64)
    yv = np.array([ground["yv"]["x"], ground["yv"]["y"]], dtype=np.float64)
    on_slope = lambda s, size: tuple(s * xv + (5.0 + size - 0.05) * yv)      # noqa: E731
    capsule = w.add_capsules(np.array([[*on_slope(80.0, 3.0), angle, 9.0, 3.0]], dtype=F))
    circle = w.add_circles(np.array([[*on_slope(-40.0, 5.0), angle, 5.0]], dtype=F))
    assert w.shapes()["kind"].tolist() == [0, 2, 1]
    start = w.bodies.copy()
    for _ in range(90):
        w.Update(DT, CFG)
    end = w.bodies
    along = lambda b: float((end["pos"]["x"][b] - start["pos"]["x"][b]) * xv[0] + (end["pos"]["y"][b] - start["pos"]["y"][b]) * xv[1])      # noqa: E731
    print("the capsule moved %.4f along the slope, the circle %.3f" % (along(capsule), along(circle)))
    assert abs(along(capsule)) < 0.5 and abs(float(end["angular_velocity"][capsule])) < 0.05
    assert abs(_angle(end, capsule) - angle) < 0.02
    assert along(circle) < -5.0, "the circle did not move downhill"


def test_six_logs_pile_up():
    w = phyx_amd.World(0, gravity=G)
    w.AddBody((0.0, 0.0), 0.0, (100.0, 10.0), static=True)
    w.AddBody((-24.0, 30.0), 0.0, (3.0, 20.0), static=True)
    w.AddBody((24.0, 30.0), 0.0, (3.0, 20.0), static=True)
    logs = [[-10.0, 14.0, 0.05, 9.0, 3.0], [10.0, 14.0, -0.04, 9.0, 3.0], [0.0, 21.0, 0.1, 9.0, 3.0],
            [-8.0, 29.0, -0.3, 9.0, 3.0], [9.0, 30.0, 0.25, 9.0, 3.0], [0.0, 38.0, 0.02, 9.0, 3.0]]
    assert w.add_capsules(np.array(logs, dtype=F)) == 3
    for _ in range(400):
        w.Update(DT, CFG)
    b = w.bodies
    speed = float(np.abs(np.stack([b["velocity"]["x"][3:], b["velocity"]["y"][3:]])).max())
    pen = _penetrations(w)
    print("largest velocity component %.4f, penetrations %.4f .. %.4f over %d points, manifold points %s" % (
        speed, pen.min(), pen.max(), len(pen), w.manifolds["point_count"].tolist()))
    assert (b["pos"]["y"][3:] > 10.0).all() and (np.abs(b["pos"]["x"][3:]) < 24.0).all(), "a log left the pen"
    assert pen.max() < 2.0, "the solver's displacement threshold is 2 units"
    assert speed < abs(G) * DT, "a pile at rest keeps less than one step of gravity"


# ---- 3. twins -----------------------------------------------------------------------------------------------------------------------------
def test_a_capsule_taken_back_steps_like_no_column():
    sc = scenes.stack(8, 8)
    a, b = phyx_amd.World(0, gravity=G), phyx_amd.World(0, gravity=G)
    a.add_scene(sc)
    b.add_scene(sc)
    size = b.bodies["geom_size"][5]
    b.set_shapes([5], SHAPE_CAPSULE, 2.0 * float(size["x"]), float(size["y"]))
    b.set_shapes([5], SHAPE_BOX, float(size["x"]), float(size["y"]))
    assert (b.shapes()["kind"] == 0).all()
    for s in range(12):
        if s == 5:                                                               # once more on the device, after steps
            b.set_shapes([9], SHAPE_CAPSULE, 2.0 * float(size["x"]), float(size["y"]))
            b.set_shapes([9], SHAPE_BOX, float(size["x"]), float(size["y"]))
        a.Update(DT, CFG)
        b.Update(DT, CFG)
        _same(a, b, "after step %d" % s)


def test_a_circle_world_that_named_a_capsule_steps_like_one_that_never_did():
    a, b = mixed_world(), mixed_world()
    sh = b.shapes()
    b.set_shapes([2], SHAPE_CAPSULE, 2.0 * float(sh["hx"][2]), float(sh["hy"][2]))
    b.set_shapes([2], int(sh["kind"][2]), float(sh["hx"][2]), float(sh["hy"][2]))
    assert b.shapes().tobytes() == a.shapes().tobytes()
    for s in range(12):
        a.Update(DT, CFG)
        b.Update(DT, CFG)
        _same(a, b, "after step %d" % s)


def test_set_state_then_set_shapes_reproduces_a_capsule_world():
    a = capsule_world()
    for _ in range(8):
        a.Update(DT, CFG)
    sh = a.shapes()
    b = phyx_amd.World(0, gravity=G)
    b.set_state(*a.state())
    assert (b.shapes()["kind"] == 0).all(), "set_state resets every kind to box"
    b.set_shapes(_all(b), sh["kind"], sh["hx"], sh["hy"])
    assert b.shapes().tobytes() == sh.tobytes()
    for s in range(8):
        a.Update(DT, CFG)
        b.Update(DT, CFG)
        _same(a, b, "step %d after the restore" % s)


def test_snapshots_carry_the_capsules():
    a = capsule_world()
    for _ in range(6):
        a.Update(DT, CFG)
    snap = a.save()
    with pytest.raises(PhxError, match="capsules") as e:
        snap.to_bytes()
    assert e.value.status == phyx_amd._lib.PHX_ERR_STATE
    b = phyx_amd.World(0, gravity=G)
    b.load(snap)
    c = a.fork()
    for w in (b, c):
        assert w.shapes().tobytes() == a.shapes().tobytes()
    for s in range(8):
        for w in (a, b, c):
            w.Update(DT, CFG)
        _same(a, b, "step %d after the load" % s)
        _same(a, c, "step %d after the fork" % s)
    with pytest.raises(PhxError, match="capsules") as e:
        a.set_shard(0, 2)
    assert e.value.status == phyx_amd._lib.PHX_ERR_STATE


# ---- 4. plumbing --------------------------------------------------------------------------------------------------------------------------
def test_removal_spawn_and_add_capsules_move_the_kinds():
    w = capsule_world()
    for _ in range(4):
        w.Update(DT, CFG)
    kinds = _kinds(w)
    gone = [3, 6, 12]
    keep = np.ones(len(kinds), dtype=bool)
    keep[gone] = False
    before = w.shapes()
    w.remove_bodies(gone)
    kinds = spec.remove(kinds, keep)
    assert _kinds(w).tolist() == kinds.tolist() and w.shapes().tobytes() == before[keep].tobytes()
    w.add_bodies(np.array([[60.0, 60.0, 0.0, 3.0, 2.0]], dtype=F))
    kinds = spec.spawn(kinds, 1)
    assert _kinds(w).tolist() == kinds.tolist()
    n = w.counts()[0]
    assert w.add_capsules(np.array([[80.0, 60.0, 0.5, 6.0, 2.0], [100.0, 60.0, 0.0, 5.0, 1.0]], dtype=F)) == n
    sh = w.shapes()
    assert sh["kind"].tolist() == kinds.tolist() + [2, 2] and sh["hx"][n:].tolist() == [6.0, 5.0] and sh["hy"][n:].tolist() == [2.0, 1.0]
    b = w.bodies
    for k, (hx, hy) in ((n, (6.0, 2.0)), (n + 1, (5.0, 1.0))):
        im, ii = spec.masses(hx, hy)
        assert b["inv_mass"][k] == im and b["inv_inertia"][k] == ii
    w.Update(DT, CFG)
    assert _kinds(w).tolist() == kinds.tolist() + [2, 2]
    # before the first step (host-staged bodies) the same calls act on the host's table
    h = phyx_amd.World(0, gravity=G)
    h.AddBody((0.0, 0.0), 0.0, (50.0, 5.0), static=True)
    assert h.add_capsules(np.array([[0.0, 6.9, 0.0, 6.0, 2.0], [20.0, 6.9, 0.0, 6.0, 2.0]], dtype=F)) == 1
    h.AddBody((40.0, 9.0), 0.0, (3.0, 3.0))
    h.remove_bodies([1])
    assert h.shapes()["kind"].tolist() == [0, 2, 0]
    h.Update(DT, CFG)
    assert h.shapes()["kind"].tolist() == [0, 2, 0] and h.manifolds["point_count"].tolist().count(2) >= 1
    with pytest.raises(ValueError):
        h.add_capsules(np.array([[0.0, 30.0, 0.0, 2.0, 2.0]], dtype=F))


def test_set_shapes_accepts_a_capsule_and_rejections_leave_the_world_unchanged():
    w = mixed_world()
    for _ in range(3):
        w.Update(DT, CFG)
    state, sh = w.state(), w.shapes()

    def unchanged(what):
        assert w.shapes().tobytes() == sh.tobytes(), what
        for name, x, y in zip(NAMES, state, w.state()):
            assert x.tobytes() == y.tobytes(), "%s changed by %s" % (name, what)

    bad = {"hx == hy": ([2], SHAPE_CAPSULE, 3.0, 3.0), "hx < hy": ([2], SHAPE_CAPSULE, 2.0, 4.0), "an infinite hx": ([2], SHAPE_CAPSULE, np.inf, 3.0),
           "a NaN hy": ([2], SHAPE_CAPSULE, 4.0, np.nan), "a zero radius": ([2], SHAPE_CAPSULE, 3.0, 0.0), "a negative size": ([2], SHAPE_CAPSULE, 3.0, -1.0),
           "a bad entry behind good ones": ([2, 4], [2, 2], [4.0, 3.0], [2.0, 3.0]), "kind 3": ([2], 3, 4.0, 2.0)}
    for what, (idx, kind, hx, hy) in bad.items():
        with pytest.raises(PhxError) as e:
            w.set_shapes(idx, kind, hx, hy)
        assert e.value.status == phyx_amd._lib.PHX_ERR_INVALID, what
        if what == "hx == hy":
            assert "use PHX_SHAPE_CIRCLE" in str(e.value)
        unchanged(what)
    w.set_shapes([2], SHAPE_CAPSULE, 4.0, 2.0)                                    # (the call this feature adds)
    got = w.shapes()[2]
    assert (int(got["kind"]), float(got["hx"]), float(got["hy"])) == (2, 4.0, 2.0)
    r = w.bodies[2]
    assert (float(r["geom_size"]["x"]), float(r["geom_size"]["y"])) == (4.0, 2.0)
    assert r["inv_mass"] == state[0][2]["inv_mass"], "the masses are not touched"
    w.Update(DT, CFG)


# ---- 5. queries on both paths -------------------------------------------------------------------------------------------------------------
def _grid(capsules=True):
    """65 bodies (one past a tree node) on a 13 x 5 grid, box / circle / capsule in turn, at angles that include 0 exactly; every fourth
    body static."""
    rows = []
    for k in range(65):
        kind = k % 3 if capsules else k % 2
        hx, hy = {0: (3.0, 2.0), 1: (2.5, 2.5), 2: (4.0, 1.5)}[kind]
        rows.append((12.0 * (k % 13) - 72.0, 10.0 * (k // 13), 0.0 if k % 5 == 0 else 0.37 * k, hx, hy, kind))
    a = np.array(rows, dtype=np.float64)
    w = phyx_amd.World(0, gravity=0.0)
    idx = w.add_bodies(a[:, :5].astype(F))
    kinds = a[:, 5].astype(np.int32)
    for kind in (SHAPE_CIRCLE, SHAPE_CAPSULE):
        sel = np.flatnonzero(kinds == kind)
        if len(sel):
            w.set_shapes(idx[sel], kind, a[sel, 3].astype(F), a[sel, 4].astype(F))
    static = idx[::4]
    w.set_inverse_masses(static, np.zeros((len(static), 2), dtype=F))
    return w


def _grid_queries(bodies, kinds):
    rng = np.random.default_rng(11)
    lo, hi = (-82.0, -8.0), (82.0, 48.0)
    pts = [rng.uniform(lo, hi, (200, 2))]
    rays, circles = [], [np.column_stack([rng.uniform(lo, hi, (120, 2)), rng.uniform(0.2, 6.0, 120)])]
    for b in np.flatnonzero(kinds == 2)[:12]:
        c = np.array([bodies["pos"]["x"][b], bodies["pos"]["y"][b]], dtype=np.float64)
        xv = np.array([bodies["xv"]["x"][b], bodies["xv"]["y"][b]], dtype=np.float64)
        yv = np.array([bodies["yv"]["x"][b], bodies["yv"]["y"][b]], dtype=np.float64)
        hx, hy = float(bodies["geom_size"]["x"][b]), float(bodies["geom_size"]["y"][b])
        a = hx - hy
        pts.append(np.array([c, c + xv * (a + 0.9 * hy), c - xv * (a + 0.9 * hy), c + xv * (hx - 0.2) + yv * (hy - 0.2), c + yv * 0.99 * hy, c + yv * 1.01 * hy]))
        for d, off in ((-yv, 0.0), (yv, 0.0), (-xv, 0.0), (xv, 0.0), (-yv, a + 0.5 * hy), (-yv, -(a + 0.5 * hy)), (-yv, hx + 0.1)):
            o = c - 4.5 * d + xv * off                                             # 4.5 away: nothing else lies between
            rays.append([*o, *d, 50.0])
        rays.append([*(c + xv * 0.5 * a), 1.0, 0.3, 20.0])                          # from inside
        rays.append([*(c - 4.5 * -yv), *(-yv), 2.0])                                # max_t short
    rays += [[x, 60.0, 0.05, -1.0, 100.0] for x in np.linspace(-80.0, 80.0, 41)]
    rays = np.array(rays, dtype=F)
    casts = np.column_stack([rays[:, 0], rays[:, 1], np.tile([0.4, 1.0, 2.5], len(rays))[:len(rays)], rays[:, 2], rays[:, 3], rays[:, 4]])
    return np.concatenate(pts).astype(F), rays, np.concatenate(circles).astype(F), casts.astype(F)


@pytest.mark.parametrize("path", ("scan", "index"))
def test_queries_see_the_capsule_on_both_paths(monkeypatch, path):
    monkeypatch.setenv("PHX_QUERY_PATH", path)
    w = _grid()
    bodies, kinds = w.bodies, _kinds(w)
    assert kinds.tolist() == [k % 3 for k in range(65)]
    pts, rays, circles, casts = _grid_queries(bodies, kinds)
    ray_parts, cast_parts = [], []
    for skip in (False, True):
        assert w.query_points(pts, skip_static=skip).tobytes() == spec.query_points(bodies, kinds, pts, skip).tobytes(), "points %s skip=%s" % (path, skip)
        got, want = w.raycast(rays, skip_static=skip), spec.raycast(bodies, kinds, rays, skip, detail=ray_parts)
        assert got.tobytes() == want.tobytes(), "rays %s skip=%s: %s" % (path, skip, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[:8])
        off, hits = w.query_circles(circles, skip_static=skip)
        woff, whits = spec.query_circles(bodies, kinds, circles, skip)
        assert off.tobytes() == woff.tobytes() and hits.tobytes() == whits.tobytes(), "circles %s skip=%s" % (path, skip)
        got, want = w.cast_circles(casts, skip_static=skip), spec.cast_circles(bodies, kinds, casts, skip, detail=cast_parts)
        assert got.tobytes() == want.tobytes(), "casts %s skip=%s: %s" % (path, skip, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[:8])
    # the spec's own answers: every part of a capsule wins, and the capsule differs from its frame box and from a disc
    assert {"side+", "side-", "end0", "end1", "inside"} <= set(ray_parts), set(ray_parts)
    assert {"side+", "side-", "end0", "end1", "inside"} <= set(cast_parts), set(cast_parts)
    assert spec.query_points(bodies, kinds, pts).tobytes() != spec.query_points(bodies, np.where(kinds == 2, 0, kinds), pts).tobytes()
    assert (np.diff(spec.query_circles(bodies, kinds, circles)[0]) > 0).any()
    # oriented boxes and box casts see the frame box
    boxes = np.array([phyx_amd.box_from_angle(x, y, 0.3, 3.0, 2.0) for x in np.linspace(-75.0, 75.0, 16) for y in (1.0, 22.0)], dtype=F)
    off, hits = w.query_boxes(boxes)
    woff, whits = sqs.query_boxes(bodies, boxes)
    assert off.tobytes() == woff.tobytes() and hits.tobytes() == whits.tobytes(), path
    bcasts = np.array([[x, 60.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.02, -1.0, 100.0] for x in np.linspace(-80.0, 80.0, 33)], dtype=F)
    assert w.cast_boxes(bcasts).tobytes() == sqs.cast_boxes(bodies, bcasts).tobytes(), path
    # the device forms
    dr, dh = DeviceBuffer(rays.nbytes), DeviceBuffer(ray_hit_dtype.itemsize * len(rays))
    dr.from_host(rays)
    w.raycast_device(dr.address(), len(rays), dh.address())
    dc, ds = DeviceBuffer(casts.nbytes), DeviceBuffer(shape_hit_dtype.itemsize * len(casts))
    dc.from_host(casts)
    w.cast_circles_device(dc.address(), len(casts), ds.address())
    dp, db = DeviceBuffer(pts.nbytes), DeviceBuffer(4 * len(pts))
    dp.from_host(pts)
    w.query_points_device(dp.address(), len(pts), db.address())
    w.sync()
    assert dh.to_host().view(ray_hit_dtype).tobytes() == spec.raycast(bodies, kinds, rays).tobytes()
    assert ds.to_host().view(shape_hit_dtype).tobytes() == spec.cast_circles(bodies, kinds, casts).tobytes()
    assert db.to_host().view(np.int32).tobytes() == spec.query_points(bodies, kinds, pts).tobytes()


@pytest.mark.parametrize("path", ("scan", "index"))
def test_a_world_of_boxes_and_circles_answers_as_before(monkeypatch, path):
    monkeypatch.setenv("PHX_QUERY_PATH", path)
    w = _grid(capsules=False)
    bodies, kinds = w.bodies, _kinds(w)
    assert set(kinds.tolist()) == {0, 1}
    pts, rays, circles, casts = _grid_queries(bodies, np.where(np.arange(65) % 3 == 2, 2, 0))
    import circle_spec
    assert w.query_points(pts).tobytes() == circle_spec.query_points(bodies, kinds, pts).tobytes()
    assert w.raycast(rays).tobytes() == circle_spec.raycast(bodies, kinds, rays).tobytes()
    off, hits = w.query_circles(circles)
    woff, whits = rqs.query_circles(bodies, kinds, circles)
    assert off.tobytes() == woff.tobytes() and hits.tobytes() == whits.tobytes()
    assert w.cast_circles(casts).tobytes() == rqs.cast_circles(bodies, kinds, casts).tobytes()
