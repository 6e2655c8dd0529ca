"""Convex polygon bodies on the device (phx_world_set_polygons; include/phyx_amd.h POLYGONS), held to tests/polygon_spec.py:
  - lockstep at the pre_solve boundary: every manifold's contact points after UpdateManifolds equal the spec's update of the previous
    step's slots on the bodies at the start of the step, byte for byte, in rows where all sixteen ordered pairs of kinds occur;
  - behaviour: a box rests on a wedge with two points and slides on a frictionless one, a triangle stood on a vertex topples, hexagons
    pile up;
  - twins: polygons named and taken back against worlds that never had the column; set_state + set_shapes + set_polygons; save / load /
    fork;
  - plumbing: removal, spawn, add_polygons; every rejection leaves the world unchanged;
  - queries on both paths against the spec: points and rays see the outline, the four shape queries the frame box."""
import numpy as np
import pytest

import capsule_spec
import phyx_amd
import polygon_spec as spec
import shape_query_spec as sqs
from phyx_amd import Configuration, DeviceBuffer, PhxError, SHAPE_BOX, SHAPE_CAPSULE, SHAPE_CIRCLE, scenes
from phyx_amd.api import contact_point_dtype, ray_hit_dtype
from test_capsules_gpu import _angle, _grid, _grid_queries, _penetrations, capsule_world
from test_circles_gpu import _all, _debug_update, _kinds, _overlapping, _same, NAMES

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)
F = np.float32

# The rows of the lockstep test.  ORDER holds every ordered pair of the four kinds as neighbours (00 01 11 12 22 23 33 30 02 20 03 31 13
# 32 21 10); the upper row is the same sequence backwards, so that every kind also meets every kind with the higher index, and rests on
# the lower one.  Boxes have the half size 4, circles the radius 4, capsules are {7, 4}; the polygons take the shapes below in turn.
ORDER = [0, 0, 1, 1, 2, 2, 3, 3, 0, 2, 0, 3, 1, 3, 2, 1, 0]
HEXAGON = spec.regular(6, 4.6)                                              # flat above and below, pointed towards its neighbours
OCTAGON = spec.regular(8, 4.4, np.pi / 8)
TRIANGLE = spec.polygon([(-5.0, -2.5), (5.0, -2.5), (0.0, 5.0)])
SHAPES = (OCTAGON, HEXAGON, TRIANGLE)                                        # (an octagon and a hexagon are the neighbours of kinds 3, 3)
WEDGE = spec.polygon([(-20.0, -3.0), (20.0, -3.0), (20.0, 5.0)])            # the slope y = 0.2 x + 1: tan = 0.2 < 0.3, the default friction
SLOPE = float(np.arctan(0.2))
SPIKE = spec.polygon([(-4.0, 2.5), (0.0, -5.0), (4.0, 2.5)])                 # a triangle with a vertex below its centre


def _verts(p):
    return np.asarray(p["v"])[:int(p["count"])]


def polygon_rows():
    """(rows {px, py, angle, hx, hy}, kinds, polygons) of the bodies above the ground."""
    rows, kinds, polys, turn = [], [], [], 0
    for order, x0, y, tilt in ((ORDER, -88.0, 10.0 + 4.0 - 0.4, -0.04), (ORDER[::-1], -84.0, 10.0 + 8.0 + 4.0 - 0.7, 0.05)):
        x = x0
        for k, kind in enumerate(order):
            p = spec.NONE
            hx, hy = {0: (4.0, 4.0), 1: (4.0, 4.0), 2: (7.0, 4.0)}.get(kind, (0.0, 0.0))
            if kind == 3:
                p = SHAPES[turn % len(SHAPES)]
                turn += 1
                hx, hy = (float(v) for v in spec.frame_box(p))
            x += hx
            rows.append((x, y, tilt + 0.03 * k if kind >= 2 else 0.1 * k, hx, hy))
            kinds.append(kind)
            polys.append(p)
            x += hx - 0.6
    return np.array(rows, dtype=np.float64), np.array(kinds, dtype=np.int32), polys


def polygon_world():
    """Body 0 the ground box, body 1 a static polygon stop at the lower row's end, then the two rows."""
    w = phyx_amd.World(0, gravity=G)
    w.AddBody((0.0, 0.0), 0.0, (200.0, 10.0), static=True)
    w.AddBody((-92.0, 14.2), 0.0, (4.0, 4.0), static=True)                      # (clear of the ground: two static bodies make no pair)
    w.set_polygons([1], OCTAGON)
    rows, kinds, polys = polygon_rows()
    idx = w.add_bodies(rows.astype(F))
    for kind, masses in ((SHAPE_CIRCLE, lambda s: phyx_amd.circle_inverse_masses(s[:, 3])), (SHAPE_CAPSULE, lambda s: phyx_amd.capsule_inverse_masses(s[:, 3], s[:, 4]))):
        sel = np.flatnonzero(kinds == kind)
        w.set_shapes(idx[sel], kind, rows[sel, 3].astype(F), rows[sel, 4].astype(F))
        w.set_inverse_masses(idx[sel], masses(rows[sel].astype(F)))
    sel = np.flatnonzero(kinds == 3)
    w.set_polygons(idx[sel], [_verts(polys[k]) for k in sel])
    w.set_inverse_masses(idx[sel], np.array([phyx_amd.polygon_inverse_masses(_verts(polys[k])) for k in sel], dtype=F))
    return w


def _polys(w):
    return list(w.polygons())


# ---- 1. lockstep at the pre_solve boundary ------------------------------------------------------------------------------------------------
def test_update_manifolds_lockstep(built_lib):
    w = polygon_world()
    kinds, polys = _kinds(w), _polys(w)
    assert kinds.tolist() == [0, 3] + ORDER + ORDER[::-1] and len(kinds) == 36
    assert w.polygons().tobytes() == np.array([spec.shown(p) for p in [spec.NONE, OCTAGON] + polygon_rows()[2]], dtype=spec.polygon_dtype).tobytes()
    prev, seen, two = {}, set(), set()
    blank = np.zeros(2, dtype=contact_point_dtype)
    blank["solver_index"] = -1
    for s in range(12):
        bodies = w.bodies
        w.PreSolve(DT)
        m, cp = w.manifolds, w.contactPoints
        now, live = {}, set()
        for k in range(len(m)):
            b1, b2 = int(m["body1"][k]), int(m["body2"][k])
            count, slots = prev.get((b1, b2), (0, blank))
            want_n, want = spec.update_manifold(bodies[b1], kinds[b1], polys[b1], bodies[b2], kinds[b2], polys[b2], count, slots) \
                if (kinds[b1] or kinds[b2]) else _debug_update(built_lib, bodies[b1], bodies[b2], count, slots)
            got_n = int(m["point_count"][k])
            got = cp[m["point_index"][k]:m["point_index"][k] + 2].copy()
            assert got_n == want_n, "step %d, pair (%d, %d) of kinds (%d, %d): %d points, the spec has %d" % (s, b1, b2, kinds[b1], kinds[b2], got_n, want_n)
            a, b = got[:got_n].copy(), want[:want_n].copy()
            a["solver_index"], b["solver_index"] = 0, 0                          # (the joint match's, not UpdateManifolds')
            assert a.tobytes() == b.tobytes(), "step %d, pair (%d, %d) of kinds (%d, %d): %s != %s" % (s, b1, b2, kinds[b1], kinds[b2], a, b)
            now[(b1, b2)] = (got_n, got)
            live.add((min(b1, b2), max(b1, b2)))
            if got_n:
                seen.add((int(kinds[b1]), int(kinds[b2])))
            if got_n == 2 and 3 in (kinds[b1], kinds[b2]):
                two.add((int(kinds[b1]), int(kinds[b2])))
        assert len(live) == len(m), "a pair has two manifolds"
        kept = {(min(a, b), max(a, b)) for (a, b), (n, _) in now.items() if (a, b) in prev and n > 0}
        assert live == _overlapping(bodies) | kept, "step %d: the manifold set is not the overlapping pairs and the live old ones" % s
        prev = now
        w.FinishStep(DT, CFG)
    print("pair kinds with points: %s; polygon pairs with two: %s" % (sorted(seen), sorted(two)))
    assert seen == {(a, b) for a in range(4) for b in range(4)}, "pair kinds with points: %s" % sorted(seen)
    assert {(3, 3), (0, 3), (3, 0)} & two, "polygon manifolds with two points: %s" % sorted(two)


# ---- 2. behaviour -----------------------------------------------------------------------------------------------------------------------
def _wedge_world(friction=None):
    """A static wedge (body 0) and a box of half size {4, 2} lying on its slope at x = 0 (body 1)."""
    w = phyx_amd.World(0, gravity=G)
    assert w.add_polygons(np.array([[0.0, 0.0, 0.0]], dtype=F), _verts(WEDGE)) == 0
    w.set_inverse_masses([0], np.zeros((1, 2), dtype=F))
    n = np.array([-np.sin(SLOPE), np.cos(SLOPE)])
    at = np.array([0.0, 1.0]) + n * (2.0 - 0.05)
    w.add_bodies(np.array([[at[0], at[1], SLOPE, 4.0, 2.0]], dtype=F))
    if friction is not None:
        w.set_materials([0, 1], friction=friction)
    return w


def _along_slope(start, end, b):
    return float((end["pos"]["x"][b] - start["pos"]["x"][b]) * np.cos(SLOPE) + (end["pos"]["y"][b] - start["pos"]["y"][b]) * np.sin(SLOPE))


def test_a_box_rests_on_a_wedge_with_two_points():
    w = _wedge_world()
    assert w.shapes()["kind"].tolist() == [3, 0]
    start = w.bodies.copy()
    for _ in range(120):
        w.Update(DT, CFG)
    end, m = w.bodies, w.manifolds
    print("the box moved %.4f along the slope, angle %.5f (slope %.5f), points %s" % (_along_slope(start, end, 1), _angle(end, 1), SLOPE, m["point_count"].tolist()))
    assert len(m) == 1 and m["point_count"].tolist() == [2]
    assert abs(_along_slope(start, end, 1)) < 0.5 and abs(_angle(end, 1) - SLOPE) < 0.02
    assert abs(float(end["angular_velocity"][1])) < 0.05 and _penetrations(w).max() < 2.0


def test_a_box_slides_on_a_frictionless_wedge():
    w = _wedge_world(friction=0.0)
    start = w.bodies.copy()
    for _ in range(40):
        w.Update(DT, CFG)
    end = w.bodies
    # a = g sin(slope) along the slope: after t = 40/60 s the box has gone g sin(slope) t^2 / 2 = 8.7 downhill
    want = 0.5 * abs(G) * np.sin(SLOPE) * (40 * DT) ** 2
    print("the box moved %.3f along the slope (free sliding: %.3f)" % (_along_slope(start, end, 1), -want))
    assert -1.3 * want < _along_slope(start, end, 1) < -0.7 * want
    assert abs(_angle(end, 1) - SLOPE) < 0.03


def test_a_triangle_stood_on_a_vertex_topples():
    w = phyx_amd.World(0, gravity=G)
    w.AddBody((0.0, 0.0), 0.0, (200.0, 10.0), static=True)
    assert w.add_polygons(np.array([[0.0, 10.0 + 5.0 - 0.1, 0.1]], dtype=F), _verts(SPIKE)) == 1
    w.Update(DT, CFG)
    assert w.manifolds["point_count"].tolist() == [1], "on its vertex a triangle has one point"
    for _ in range(299):
        w.Update(DT, CFG)
    b = w.bodies
    print("angle %.4f, height %.4f, points %s" % (_angle(b, 1), float(b["pos"]["y"][1]), w.manifolds["point_count"].tolist()))
    # its faces lie 2.5 and 2.35 from its centre
    assert w.manifolds["point_count"].tolist() == [2] and 11.5 < float(b["pos"]["y"][1]) < 12.6
    assert abs(float(b["angular_velocity"][1])) < 0.05


def test_hexagons_pile_up():
    w = phyx_amd.World(0, gravity=G)
    w.AddBody((0.0, 0.0), 0.0, (100.0, 10.0), static=True)
    w.AddBody((-22.0, 30.0), 0.0, (3.0, 20.0), static=True)
    w.AddBody((22.0, 30.0), 0.0, (3.0, 20.0), static=True)
    spawn = [[-9.0, 14.5, 0.05], [9.0, 14.5, -0.04], [0.0, 22.5, 0.1], [-9.0, 31.0, -0.3], [9.0, 31.5, 0.25], [0.0, 40.0, 0.02]]
    assert w.add_polygons(np.array(spawn, dtype=F), _verts(HEXAGON)) == 3
    for _ in range(400):
        w.Update(DT, CFG)
    b = w.bodies
    speed = float(np.abs(np.stack([b["velocity"]["x"][3:], b["velocity"]["y"][3:]])).max())
    pen = _penetrations(w)
    print("largest velocity component %.4f, penetrations %.4f .. %.4f over %d points, manifold points %s" % (
        speed, pen.min(), pen.max(), len(pen), w.manifolds["point_count"].tolist()))
    assert (b["pos"]["y"][3:] > 10.0).all() and (np.abs(b["pos"]["x"][3:]) < 22.0).all(), "a hexagon left the pen"
    assert pen.max() < 2.0, "the solver's displacement threshold is 2 units"
    assert speed < abs(G) * DT, "a pile at rest keeps less than one step of gravity"


# ---- 3. twins -----------------------------------------------------------------------------------------------------------------------------
def _corners(size):
    hx, hy = float(size["x"]), float(size["y"])
    return [(-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy)]


def test_polygons_taken_back_step_like_no_column():
    sc = scenes.stack(8, 8)
    a, b = phyx_amd.World(0, gravity=G), phyx_amd.World(0, gravity=G)
    a.add_scene(sc)
    b.add_scene(sc)
    size = b.bodies["geom_size"][5]
    b.set_polygons([5], _corners(size))
    assert b.shapes()["kind"][5] == 3 and b.polygons([5])["count"].tolist() == [4]
    b.set_shapes([5], SHAPE_BOX, float(size["x"]), float(size["y"]))
    assert (b.shapes()["kind"] == 0).all() and not b.polygons()["count"].any(), "set_shapes resets the polygon record"
    for s in range(12):
        if s == 5:                                                               # once more on the device, after steps
            b.set_polygons([9, 11], _corners(size))
            b.set_shapes([9, 11], SHAPE_BOX, float(size["x"]), float(size["y"]))
            assert not b.polygons()["count"].any()
        a.Update(DT, CFG)
        b.Update(DT, CFG)
        _same(a, b, "after step %d" % s)


def test_a_capsule_world_that_named_a_polygon_steps_like_one_that_never_did():
    a, b = capsule_world(), capsule_world()
    sh = b.shapes()
    for body in (2, 4, 5):                                                       # a circle, a capsule, a box
        b.set_polygons([body], _verts(HEXAGON))
        b.set_shapes([body], int(sh["kind"][body]), float(sh["hx"][body]), float(sh["hy"][body]))
    assert b.shapes().tobytes() == a.shapes().tobytes()
    for s in range(12):
        a.Update(DT, CFG)
        b.Update(DT, CFG)
        _same(a, b, "after step %d" % s)


def _restore_shapes(b, sh, polys):
    rest = np.flatnonzero(sh["kind"] != 3).astype(np.int32)
    b.set_shapes(rest, sh["kind"][rest], sh["hx"][rest], sh["hy"][rest])
    named = np.flatnonzero(sh["kind"] == 3).astype(np.int32)
    b.set_polygons(named, polys[named])


def test_set_state_then_set_shapes_and_set_polygons_reproduce_a_polygon_world():
    a = polygon_world()
    for _ in range(6):
        a.Update(DT, CFG)
    sh, polys = a.shapes(), a.polygons()
    b = phyx_amd.World(0, gravity=G)
    b.set_state(*a.state())
    assert (b.shapes()["kind"] == 0).all() and not b.polygons()["count"].any(), "set_state resets every kind to box and drops the column"
    assert _all(b).tolist() == list(range(36))
    _restore_shapes(b, sh, polys)
    assert b.shapes().tobytes() == sh.tobytes() and b.polygons().tobytes() == polys.tobytes()
    for s in range(6):
        a.Update(DT, CFG)
        b.Update(DT, CFG)
        _same(a, b, "step %d after the restore" % s)
    # a polygon set before the first step and one set after it are the same bytes: c is built on the host, d on the device
    c, e, d = phyx_amd.World(0, gravity=G), phyx_amd.World(0, gravity=G), phyx_amd.World(0, gravity=G)
    for w in (c, e):
        w.AddBody((0.0, 0.0), 0.0, (60.0, 10.0), static=True)
        w.AddBody((0.0, 14.4), 0.3, (4.6, 4.6))
    d.set_state(*e.state())                                                      # (set_state puts the bodies on the device)
    c.set_polygons([1], _verts(OCTAGON))                                         # host-staged
    d.set_polygons([1], _verts(OCTAGON))                                         # on the device
    assert c.polygons().tobytes() == d.polygons().tobytes() and c.shapes().tobytes() == d.shapes().tobytes()
    for s in range(5):
        c.Update(DT, CFG)
        d.Update(DT, CFG)
        _same(c, d, "host-set against device-set, step %d" % s)


def test_snapshots_carry_the_polygons():
    a = polygon_world()
    for _ in range(5):
        a.Update(DT, CFG)
    snap = a.save()
    with pytest.raises(PhxError, match="polygons") as e:
        snap.to_bytes()
    assert e.value.status == phyx_amd._lib.PHX_ERR_STATE
    b = phyx_amd.World(0, gravity=G)
    b.load(snap)
    c = a.fork()
    for w in (b, c):
        assert w.shapes().tobytes() == a.shapes().tobytes() and w.polygons().tobytes() == a.polygons().tobytes()
    for s in range(6):
        for w in (a, b, c):
            w.Update(DT, CFG)
        _same(a, b, "step %d after the load" % s)
        _same(a, c, "step %d after the fork" % s)
    with pytest.raises(PhxError, match="polygons") as e:
        a.set_shard(0, 2)
    assert e.value.status == phyx_amd._lib.PHX_ERR_STATE


# ---- 4. plumbing --------------------------------------------------------------------------------------------------------------------------
def test_removal_spawn_and_add_polygons_move_the_polygons():
    w = polygon_world()
    for _ in range(3):
        w.Update(DT, CFG)
    kinds, polys = _kinds(w), _polys(w)
    gone = [3, 8, 9, 20]
    assert kinds[8] == 3 and kinds[9] == 3
    keep = np.ones(len(kinds), dtype=bool)
    keep[gone] = False
    before, before_polys = w.shapes(), w.polygons()
    w.remove_bodies(gone)
    kinds, polys = capsule_spec.remove(kinds, keep), spec.remove(polys, keep)
    assert _kinds(w).tolist() == kinds.tolist() and w.shapes().tobytes() == before[keep].tobytes()
    assert w.polygons().tobytes() == before_polys[keep].tobytes() == np.array(polys, dtype=spec.polygon_dtype).tobytes()
    w.add_bodies(np.array([[60.0, 80.0, 0.0, 3.0, 2.0]], dtype=F))
    kinds, polys = capsule_spec.spawn(kinds, 1), spec.spawn(polys, 1)
    assert _kinds(w).tolist() == kinds.tolist() and int(w.polygons()["count"][-1]) == 0
    n = w.counts()[0]
    assert w.add_polygons(np.array([[80.0, 80.0, 0.5], [100.0, 80.0, 0.0]], dtype=F), [_verts(TRIANGLE), _verts(OCTAGON)]) == n
    sh, got = w.shapes(), w.polygons()
    assert sh["kind"].tolist() == kinds.tolist() + [3, 3]
    assert got[n:].tobytes() == np.array([spec.shown(TRIANGLE), spec.shown(OCTAGON)], dtype=spec.polygon_dtype).tobytes()
    assert (sh["hx"][n], sh["hy"][n]) == spec.frame_box(TRIANGLE) and (sh["hx"][n + 1], sh["hy"][n + 1]) == spec.frame_box(OCTAGON)
    b = w.bodies
    for k, p in ((n, TRIANGLE), (n + 1, OCTAGON)):
        im, ii = spec.masses(_verts(p))
        assert b["inv_mass"][k] == im and b["inv_inertia"][k] == ii
    w.Update(DT, CFG)
    assert _kinds(w).tolist() == kinds.tolist() + [3, 3]
    # before the first step (host-staged bodies) the same calls act on the host's tables
    h = phyx_amd.World(0, gravity=G)
    h.AddBody((0.0, 0.0), 0.0, (50.0, 5.0), static=True)
    assert h.add_polygons(np.array([[0.0, 8.9, 0.0], [20.0, 8.9, 0.0]], dtype=F), _verts(HEXAGON)) == 1
    h.AddBody((40.0, 9.0), 0.0, (3.0, 3.0))
    h.remove_bodies([1])
    assert h.shapes()["kind"].tolist() == [0, 3, 0] and h.polygons()["count"].tolist() == [0, 6, 0]
    h.Update(DT, CFG)
    assert h.shapes()["kind"].tolist() == [0, 3, 0] and h.manifolds["point_count"].tolist().count(2) >= 1
    with pytest.raises(ValueError):
        h.add_polygons(np.array([[0.0, 30.0, 0.0]], dtype=F), [[(0.0, 0.0), (1.0, 0.0)]])


def test_rejections_leave_the_world_unchanged():
    w = polygon_world()
    for _ in range(3):
        w.Update(DT, CFG)
    state, sh, polys = w.state(), w.shapes(), w.polygons()

    def unchanged(what):
        assert w.shapes().tobytes() == sh.tobytes() and w.polygons().tobytes() == polys.tobytes(), what
        for name, x, y in zip(NAMES, state, w.state()):
            assert x.tobytes() == y.tobytes(), "%s changed by %s" % (name, what)

    sq = np.array([(-4, -4), (4, -4), (4, 4), (-4, 4)], dtype=np.float64)
    ok = sq.tolist()
    bad = {"clockwise": ([2], [sq[::-1].tolist()]), "origin outside": ([2], [(sq + 5.0).tolist()]), "origin on an edge": ([2], [(sq + (4.0, 0.0)).tolist()]),
           "collinear": ([2], [[(-4, -4), (0, -4), (4, -4), (4, 4), (-4, 4)]]), "concave": ([2], [[(-4, -4), (4, -4), (1, 0), (4, 4), (-4, 4)]]),
           "two vertices": ([2], [sq[:2].tolist()]), "a NaN": ([2], [[(-4, -4), (4, np.nan), (4, 4), (-4, 4)]]),
           "an infinity": ([2], [[(-4, -4), (np.inf, -4), (4, 4), (-4, 4)]]), "a bad entry behind good ones": ([2, 4], [ok, sq[::-1].tolist()]),
           "a body twice": ([2, 2], [ok, ok]), "an index out of range": ([len(sh)], [ok])}
    for what, (idx, p) in bad.items():
        assert all(spec.poly_valid(spec.polygon(v)) for v in p) == (what in ("a body twice", "an index out of range")), what
        with pytest.raises(PhxError) as e:
            w.set_polygons(idx, p)
        assert e.value.status == phyx_amd._lib.PHX_ERR_INVALID, what
        unchanged(what)
    nine = np.zeros(1, dtype=spec.polygon_dtype)
    nine["count"] = 9
    with pytest.raises(PhxError) as e:
        w.set_polygons([2], nine)
    assert e.value.status == phyx_amd._lib.PHX_ERR_INVALID
    unchanged("nine vertices")
    with pytest.raises(PhxError, match="phx_world_set_polygons") as e:          # set_shapes keeps refusing kind 3 and names the call
        w.set_shapes([2], 3, 4.0, 4.0)
    assert e.value.status == phyx_amd._lib.PHX_ERR_INVALID
    unchanged("set_shapes with kind 3")
    w.PreSolve(DT)
    with pytest.raises(PhxError) as e:
        w.set_polygons([2], ok)
    assert e.value.status == phyx_amd._lib.PHX_ERR_STATE
    w.FinishStep(DT, CFG)
    junk = spec.polygon(ok)
    junk["v"][5] = (np.nan, 7.0)                                                 # unused slots are not read, and are stored as +0
    w.set_polygons([2], junk)
    assert w.polygons([2]).tobytes() == np.array([spec.shown(spec.polygon(ok))]).tobytes()
    got = w.shapes()[2]
    assert (int(got["kind"]), float(got["hx"]), float(got["hy"])) == (3, 4.0, 4.0)
    assert w.bodies[2]["inv_mass"] == state[0][2]["inv_mass"], "the masses are not touched"
    w.Update(DT, CFG)


# ---- 5. queries on both paths -------------------------------------------------------------------------------------------------------------
def _polygon_grid():
    """test_capsules_gpu's grid of 65 bodies with every fourth kind a polygon: box / circle / capsule / polygon in turn."""
    rows, polys = [], []
    for k in range(65):
        kind = k % 4
        p = SHAPES[(k // 4) % 3] if kind == 3 else spec.NONE
        hx, hy = {0: (3.0, 2.0), 1: (2.5, 2.5), 2: (4.0, 1.5)}[kind] if kind != 3 else (float(v) for v in spec.frame_box(p))
        rows.append((14.0 * (k % 13) - 84.0, 13.0 * (k // 13), 0.0 if k % 5 == 0 else 0.37 * k, hx, hy, kind))
        polys.append(p)
    a = np.array(rows, dtype=np.float64)
    w = phyx_amd.World(0, gravity=0.0)
    idx = w.add_bodies(a[:, :5].astype(F))
    kinds = a[:, 5].astype(np.int32)
    for kind in (SHAPE_CIRCLE, SHAPE_CAPSULE):
        sel = np.flatnonzero(kinds == kind)
        w.set_shapes(idx[sel], kind, a[sel, 3].astype(F), a[sel, 4].astype(F))
    sel = np.flatnonzero(kinds == 3)
    w.set_polygons(idx[sel], [_verts(polys[k]) for k in sel])
    static = idx[::4]
    w.set_inverse_masses(static, np.zeros((len(static), 2), dtype=F))
    return w, polys


def _polygon_queries(bodies, kinds, polys):
    rng = np.random.default_rng(12)
    lo, hi = (-96.0, -10.0), (96.0, 64.0)
    pts, rays = [rng.uniform(lo, hi, (200, 2))], []
    for b in np.flatnonzero(kinds == 3)[:12]:
        c = np.array([bodies["pos"]["x"][b], bodies["pos"]["y"][b]], dtype=np.float64)
        xv = np.array([bodies["xv"]["x"][b], bodies["xv"]["y"][b]], dtype=np.float64)
        yv = np.array([bodies["yv"]["x"][b], bodies["yv"]["y"][b]], dtype=np.float64)
        hx, hy = float(bodies["geom_size"]["x"][b]), float(bodies["geom_size"]["y"][b])
        world = [c + xv * x + yv * y for x, y in _verts(polys[b]).astype(np.float64)]
        # the centre, just inside and just outside every vertex, the frame box's corners (outside the outline but by a triangle's base)
        pts.append(np.array([c] + [c + 0.97 * (v - c) for v in world] + [c + 1.03 * (v - c) for v in world] +
                            [c + sx * 0.97 * hx * xv + sy * 0.97 * hy * yv for sx in (-1, 1) for sy in (-1, 1)]))
        for k in range(len(world)):                                               # down onto every edge's middle, and along the frame's axes
            mid = 0.5 * (world[k] + world[(k + 1) % len(world)])
            d = (c - mid) / np.hypot(*(c - mid))
            rays.append([*(mid - 3.0 * d), *d, 50.0])
        for d in (xv, -xv, yv, -yv):
            rays.append([*(c - 6.5 * d), *d, 50.0])
        rays.append([*c, 1.0, 0.3, 20.0])                                         # from inside
        rays.append([*(c - 6.5 * yv), *yv, 1.0])                                  # max_t short
        rays.append([*(c - 6.5 * yv + 0.98 * hx * xv), *yv, 50.0])                # through the frame box's edge: misses a pointed polygon
    rays += [[x, 70.0, 0.05, -1.0, 100.0] for x in np.linspace(-90.0, 90.0, 41)]
    return np.concatenate(pts).astype(F), np.array(rays, dtype=F)


@pytest.mark.parametrize("path", ("scan", "index"))
def test_queries_see_the_polygon_on_both_paths(monkeypatch, path):
    monkeypatch.setenv("PHX_QUERY_PATH", path)
    w, polys = _polygon_grid()
    bodies, kinds = w.bodies, _kinds(w)
    assert kinds.tolist() == [k % 4 for k in range(65)]
    assert w.polygons().tobytes() == np.array([spec.shown(p) for p in polys], dtype=spec.polygon_dtype).tobytes()
    pts, rays = _polygon_queries(bodies, kinds, polys)
    boxed = spec.as_frame_boxes(kinds)
    for skip in (False, True):
        assert w.query_points(pts, skip_static=skip).tobytes() == spec.query_points(bodies, kinds, polys, pts, skip).tobytes(), "points %s skip=%s" % (path, skip)
        got, want = w.raycast(rays, skip_static=skip), spec.raycast(bodies, kinds, polys, rays, skip)
        assert got.tobytes() == want.tobytes(), "rays %s skip=%s: %s" % (path, skip, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[:8])
    # the spec's own answers: the outline differs from the frame box, for points and for rays, and polygons are hit
    want = spec.raycast(bodies, kinds, polys, rays)
    assert spec.query_points(bodies, kinds, polys, pts).tobytes() != capsule_spec.query_points(bodies, boxed, pts).tobytes()
    assert want.tobytes() != capsule_spec.raycast(bodies, boxed, rays).tobytes()
    hit = want["body"][want["body"] >= 0]
    assert (kinds[hit] == 3).sum() >= 60 and (want["t"][want["body"] >= 0][kinds[hit] == 3] == 0).any(), "a ray from inside a polygon"
    # the four shape queries see the frame box
    rng = np.random.default_rng(13)
    circles = np.column_stack([rng.uniform((-96.0, -10.0), (96.0, 64.0), (150, 2)), rng.uniform(0.2, 6.0, 150)]).astype(F)
    casts = np.column_stack([rays[:, 0], rays[:, 1], np.tile([0.4, 1.0, 2.5], len(rays))[:len(rays)], rays[:, 2], rays[:, 3], rays[:, 4]]).astype(F)
    off, hits = w.query_circles(circles)
    woff, whits = capsule_spec.query_circles(bodies, boxed, circles)
    assert off.tobytes() == woff.tobytes() and hits.tobytes() == whits.tobytes(), "circles %s" % path
    got, want = w.cast_circles(casts), capsule_spec.cast_circles(bodies, boxed, casts)
    assert got.tobytes() == want.tobytes(), "circle casts %s: %s" % (path, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[:8])
    boxes = np.array([phyx_amd.box_from_angle(x, y, 0.3, 3.0, 2.0) for x in np.linspace(-88.0, 88.0, 16) for y in (1.0, 27.0)], dtype=F)
    off, hits = w.query_boxes(boxes)
    woff, whits = sqs.query_boxes(bodies, boxes)
    assert off.tobytes() == woff.tobytes() and hits.tobytes() == whits.tobytes(), path
    bcasts = np.array([[x, 70.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.02, -1.0, 100.0] for x in np.linspace(-90.0, 90.0, 33)], dtype=F)
    assert w.cast_boxes(bcasts).tobytes() == sqs.cast_boxes(bodies, bcasts).tobytes(), path
    # the device forms
    dr, dh = DeviceBuffer(rays.nbytes), DeviceBuffer(ray_hit_dtype.itemsize * len(rays))
    dr.from_host(rays)
    w.raycast_device(dr.address(), len(rays), dh.address())
    dp, db = DeviceBuffer(pts.nbytes), DeviceBuffer(4 * len(pts))
    dp.from_host(pts)
    w.query_points_device(dp.address(), len(pts), db.address())
    w.sync()
    assert dh.to_host().view(ray_hit_dtype).tobytes() == spec.raycast(bodies, kinds, polys, rays).tobytes()
    assert db.to_host().view(np.int32).tobytes() == spec.query_points(bodies, kinds, polys, pts).tobytes()


@pytest.mark.parametrize("path", ("scan", "index"))
def test_a_world_without_polygons_answers_as_before(monkeypatch, path):
    """The capsule grid, plain and after a polygon was named and taken back (the polygon instantiations answer for a world that holds
    none): both give the capsule spec's bytes."""
    monkeypatch.setenv("PHX_QUERY_PATH", path)
    for named in (False, True):
        w = _grid()
        if named:
            sh = w.shapes()
            w.set_polygons([6], _verts(HEXAGON))
            w.set_shapes([6], int(sh["kind"][6]), float(sh["hx"][6]), float(sh["hy"][6]))
            assert w.shapes().tobytes() == sh.tobytes()
        bodies, kinds = w.bodies, _kinds(w)
        pts, rays, circles, casts = _grid_queries(bodies, kinds)
        assert w.query_points(pts).tobytes() == capsule_spec.query_points(bodies, kinds, pts).tobytes(), named
        assert w.raycast(rays).tobytes() == capsule_spec.raycast(bodies, kinds, rays).tobytes(), named
        off, hits = w.query_circles(circles)
        woff, whits = capsule_spec.query_circles(bodies, kinds, circles)
        assert off.tobytes() == woff.tobytes() and hits.tobytes() == whits.tobytes(), named
        assert w.cast_circles(casts).tobytes() == capsule_spec.cast_circles(bodies, kinds, casts).tobytes(), named
