"""Continuous bodies on the device (phx_world_set_continuous; include/phyx_amd.h CONTINUOUS BODIES), held to tests/sweep_spec.py:
  - lockstep: the corpus' worlds, and rows of targets at the lane-stride loop's edges under more waves than a workgroup holds, are
    stepped on the device; sweep_hits and the body states equal the specification's byte for byte;
  - it does what it is for: a marble, a box, a capsule and a hexagon at 120 units/s against a thin wall and a static triangle's slope;
    the discrete twin (the control) ends beyond both, the continuous body in front with a manifold within two steps;
  - it does nothing where nothing is fast: a settling pile with every body continuous equals its twin without the column;
  - no sticking: a pushed box travels as far as its twin, a clamped body keeps moving sideways;
  - plumbing: the column through spawn, removal, set_state, save / load / fork, export / import; the calls' refusals."""
import ctypes as C

import numpy as np
import pytest

import phyx_amd
import polygon_spec as ps
import query_corpus as qc
import sweep_corpus as sc
import sweep_spec as spec
from phyx_amd import Configuration, PhxError, SHAPE_BOX, SHAPE_CAPSULE, SHAPE_CIRCLE, SHAPE_POLYGON, Snapshot

pytestmark = pytest.mark.gpu

F = np.float32
DT = sc.DT
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)
STATIC = np.zeros((1, 2), dtype=F)


def _verts(p):
    return np.asarray(p["v"])[:int(p["count"])]


def build(bodies, kinds, polys, static, start=None, gravity=0.0):
    """A device world of the records' bodies (positions from `start` where given): add_bodies, the exact frames, the shapes, the polygons,
    the static ones' masses."""
    w = phyx_amd.World(0, gravity=gravity)
    n = len(bodies)
    b = bodies.copy()
    if start is not None:
        b["pos"]["x"], b["pos"]["y"] = start[:, 0], start[:, 1]
    rows = np.stack([b["pos"]["x"], b["pos"]["y"], np.zeros(n), b["geom_size"]["x"], b["geom_size"]["y"]], axis=1).astype(F)
    idx = w.add_bodies(rows)
    w.set_poses(idx, qc.frames(b))
    for kind in (SHAPE_CIRCLE, SHAPE_CAPSULE):
        sel = np.flatnonzero(np.asarray(kinds) == kind).astype(np.int32)
        if len(sel):
            w.set_shapes(sel, kind, b["geom_size"]["x"][sel], b["geom_size"]["y"][sel])
    sel = np.flatnonzero(np.asarray(kinds) == SHAPE_POLYGON).astype(np.int32)
    if len(sel):
        w.set_polygons(sel, [_verts(polys[k]) for k in sel])
    sel = np.flatnonzero(static).astype(np.int32)
    if len(sel):
        w.set_inverse_masses(sel, np.zeros((len(sel), 2), dtype=F))
    return w


def _polys(w):
    return list(w.polygons()) if (w.shapes()["kind"] == SHAPE_POLYGON).any() else None


def lockstep(w, steps, flags=None, filters=None, exclusions=None, dt=DT):
    """Step w `steps` times.  Before each step a fork of w is made discrete: it is the control, and its bodies behind the step are what
    IntegratePosition gave w's.  w's bodies and sweep_hits must then be the specification's pass on them, byte for byte.  Returns the
    hits of every step."""
    kinds, polys = w.shapes()["kind"], _polys(w)
    taken = []
    for s in range(steps):
        rc = w.continuous()
        before = w.bodies
        twin = w.fork()
        twin.set_continuous(np.flatnonzero(rc > 0).astype(np.int32), 0.0)
        assert twin.bodies.tobytes() == before.tobytes()
        twin.Update(dt, CFG)
        w.Update(dt, CFG)
        assert twin.sweep_counts() == (0, 0), "the control launched a pass"
        start = np.stack([before["pos"]["x"], before["pos"]["y"]], axis=1)
        want, want_hits = spec.sweep(twin.bodies, start, rc, kinds, polys, flags, filters, exclusions)
        got, got_hits = w.bodies, w.sweep_hits()
        assert got_hits.tobytes() == want_hits.tobytes(), "step %d: hits %s, the spec has %s" % (s, got_hits, want_hits)
        assert got.tobytes() == want.tobytes(), "step %d: bodies %s differ" % (s, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)]))
        taken.append(got_hits)
    return taken


# ---- 1. lockstep ------------------------------------------------------------------------------------------------------------------------
def corpus_world():
    """Every corpus case in one world, case k shifted by (96 k, 0) (its own coordinates stay small; the cases are too far apart to see
    each other): (world, flags, filters, exclusions, the cases' first body)."""
    import filter_spec
    records, kinds, polys, start, rc, first = [], [], [], [], [], []
    flags, filters, excl = [], [], []
    at = 0
    for k, c in enumerate(sc.cases()):
        b = c.bodies.copy()
        shift = F(96.0 * k)
        b["pos"]["x"] = (b["pos"]["x"] + shift).astype(F)
        records.append(b)
        kinds.append(c.kinds)
        polys += c.polys
        s = c.start.copy()
        s[:, 0] = (s[:, 0] + shift).astype(F)
        start.append(s)
        rc.append(c.rc)
        n = len(b)
        flags.append(np.zeros(n, dtype=np.uint32) if c.flags is None else c.flags)
        filters.append(filter_spec.filters(n) if c.filters is None else c.filters)
        if c.exclusions is not None:
            excl.append(np.asarray(c.exclusions, dtype=np.int32) + at)
        first.append(at)
        at += n
    records, kinds, start, rc = np.concatenate(records), np.concatenate(kinds), np.concatenate(start), np.concatenate(rc)
    flags, filters, excl = np.concatenate(flags), np.concatenate(filters), np.concatenate(excl)
    records["index"] = np.arange(len(records))
    static = (records["inv_mass"] == 0) & (records["inv_inertia"] == 0)
    w = build(records, kinds, polys, static, start)
    movers = np.flatnonzero(rc > 0).astype(np.int32)
    d = np.stack([records["pos"]["x"][movers] - start[movers, 0], records["pos"]["y"][movers] - start[movers, 1]], axis=1).astype(F)
    w.set_velocities(movers, np.column_stack([d / F(DT), np.zeros(len(movers), dtype=F)]).astype(F))
    every = np.arange(len(records), dtype=np.int32)
    w.set_body_flags(every, flags)
    w.set_collision_filters(every, filters["category"], filters["mask"], filters["group"])
    w.add_collision_exclusions(excl)
    # (the swept bodies are circles: their inradius is their radius)
    w.set_continuous(movers, rc[movers])
    return w, flags, filters, excl, first


def test_the_corpus_in_lockstep(built_lib):
    w, flags, filters, excl, first = corpus_world()
    cases = sc.cases()
    assert w.counts()[0] == sum(len(c.bodies) for c in cases)
    hits = lockstep(w, 1, flags, filters, excl)[0]
    by_body = {int(h["body"]): h for h in hits}
    m = w.manifolds
    m = m[m["point_count"] > 0]                                            # (an outline that overlapped a target at the start: the solver had its say in e)
    in_contact = set(m["body1"].tolist()) | set(m["body2"].tolist())
    clamped = 0
    for k, c in enumerate(cases):
        if first[k] + c.mover in in_contact:
            continue
        h = by_body.get(first[k] + c.mover)
        if c.want[0] is None:
            assert h is None, "%s: clamped against %s" % (c.name, h)
        else:
            assert h is not None and int(h["target"]) == first[k] + c.want[0], "%s: %s" % (c.name, h)
            clamped += 1
    assert clamped >= 100
    assert w.sweep_counts() == (1, len(hits))
    assert (np.diff(hits["body"]) > 0).all(), "ascending by body"


def stride_world(targets, movers):
    """`targets` static bodies of the four kinds in turn in a row, 8 apart, and `movers` swept circles above it: mover m is aimed straight
    down at target 7 m mod targets if m is even, at the gap behind it if m is odd.  Bodies: the targets, then the movers."""
    rows, polys = [], []
    shapes = {0: (2.0, 1.0), 1: (1.5, 1.5), 2: (2.0, 0.75)}
    for j in range(targets):
        kind = j % 4
        poly = ps.NONE
        if kind == 3:
            poly = sc.OCTAGON if j % 8 == 3 else sc.TRIANGLE
            hx, hy = (float(v) for v in ps.frame_box(poly))
        else:
            hx, hy = shapes[kind]
        rows.append((8.0 * j, 0.0, 0.3 * j, hx, hy, kind))
        polys.append(poly)
    for m in range(movers):
        j = (7 * m) % targets
        rows.append((8.0 * j + (4.0 if m % 2 else 0.3), 4.0, "0", sc.R, sc.R, SHAPE_CIRCLE))
        polys.append(ps.NONE)
    records, kinds = qc.records(rows)
    static = np.arange(len(rows)) < targets
    w = build(records, kinds, polys, static)
    idx = np.arange(targets, targets + movers, dtype=np.int32)
    w.set_velocities(idx, np.tile(np.array([[0.0, -3.5 / DT, 0.0]], dtype=F), (movers, 1)))
    w.set_continuous(idx)                                                   # (factor 0.8 of the radius 0.5: rc = 0.4)
    assert w.continuous()[idx].tobytes() == (F(0.8) * np.full(movers, sc.R, dtype=F)).astype(F).tobytes()
    return w


@pytest.mark.parametrize("targets, movers", [(1, 1), (63, 4), (64, 5), (65, 5), (129, 70)])
def test_rows_of_targets_in_lockstep(built_lib, targets, movers):
    """The lane-stride loop's edges (1, 63, 64, 65, 129 bodies and the movers behind them), and 1, 4, 5 and 70 waves: more than a
    workgroup holds, more than one word of the ordered compaction."""
    w = stride_world(targets, movers)
    taken = lockstep(w, 3)
    aimed = (movers + 1) // 2
    assert len(taken[0]) == aimed and sorted(taken[0]["body"].tolist()) == [targets + m for m in range(0, movers, 2)]
    assert taken[0]["target"].tolist() == [(7 * m) % targets for m in range(0, movers, 2)]
    assert w.sweep_counts()[0] == 3


# ---- 2. it does what it is for ----------------------------------------------------------------------------------------------------------
HEXAGON = ps.regular(6, 0.3)
MOVERS = {"marble": (SHAPE_CIRCLE, 0.25, 0.25, None), "box": (SHAPE_BOX, 0.25, 0.25, None), "capsule": (SHAPE_CAPSULE, 0.5, 0.25, None), "hexagon": (SHAPE_POLYGON, 0.3, 0.3, HEXAGON)}
SLOPE = ps.polygon([(-0.6, -0.3), (0.6, -0.3), (0.0, 0.6)])                 # thin: 120 units/s carries a body through it in one step
STEP = 1.0 / 60.0


def _obstacle_world(obstacle, mover, continuous):
    """Body 0: the obstacle, static: a wall of half thickness 0.25 at x = 0, or SLOPE at the origin.  Body 1: the mover at 120 units/s
    along -n of the face it is aimed at.  Returns (world, the unit direction of flight, the face's outward normal n, a point on the face)."""
    w = phyx_amd.World(0, gravity=0.0)
    if obstacle == "wall":
        w.add_bodies(np.array([[0.0, 0.0, 0.0, 0.25, 5.0]], dtype=F))
        n, on = np.array([-1.0, 0.0]), np.array([-0.25, 0.3])
    else:
        w.add_polygons(np.array([[0.0, 0.0, 0.0]], dtype=F), _verts(SLOPE))
        n, on = np.array([-3.0, 2.0]) / np.sqrt(13.0), np.array([-0.3, 0.15])  # the left slope, from (0, 0.6) down to (-0.6, -0.3), at its middle
    w.set_inverse_masses([0], STATIC)
    kind, hx, hy, poly = MOVERS[mover]
    at = on + n * 0.55
    if poly is not None:
        w.add_polygons(np.array([[at[0], at[1], 0.0]], dtype=F), _verts(poly))
    else:
        w.add_bodies(np.array([[at[0], at[1], 0.0, hx, hy]], dtype=F))
        if kind != SHAPE_BOX:
            w.set_shapes([1], kind, hx, hy)
    w.set_velocities([1], np.array([[-120.0 * n[0], -120.0 * n[1], 0.0]], dtype=F))
    if continuous:
        w.set_continuous([1])
    return w, -n, n, on


def _touching(w, a, b):
    m = w.manifolds
    pair = ((m["body1"] == a) & (m["body2"] == b)) | ((m["body1"] == b) & (m["body2"] == a))
    return bool((pair & (m["point_count"] > 0)).any())


@pytest.mark.parametrize("obstacle", ["wall", "slope"])
@pytest.mark.parametrize("mover", sorted(MOVERS))
def test_a_fast_body_does_not_tunnel(built_lib, obstacle, mover):
    # the control: the discrete twin ends beyond the obstacle and never touched it
    w, fly, n, on = _obstacle_world(obstacle, mover, False)
    touched = False
    for _ in range(4):
        w.Update(STEP, CFG)
        touched = touched or _touching(w, 0, 1)
    p = np.array([w.bodies[1]["pos"]["x"], w.bodies[1]["pos"]["y"]], dtype=np.float64)
    assert (p - on) @ n < -2.0 and not touched and w.sweep_counts() == (0, 0), "the control did not tunnel: %s" % p
    # the continuous body: stopped at the face, a manifold within two steps, in front of it for good
    w, fly, n, on = _obstacle_world(obstacle, mover, True)
    rc = float(w.continuous()[1])
    assert 0.0 < rc < float(w.inradii([1])[0])
    w.Update(STEP, CFG)
    hits = w.sweep_hits()
    assert len(hits) == 1 and hits[0]["body"] == 1 and hits[0]["target"] == 0 and 0.0 < hits[0]["t"] < 1.0, hits
    assert np.abs(np.asarray(hits[0]["normal"], dtype=np.float64) - n).max() < 1e-5
    p = np.array([w.bodies[1]["pos"]["x"], w.bodies[1]["pos"]["y"]], dtype=np.float64)
    assert abs((p - on) @ n - rc * (1.0 + 1.0 / 64.0)) < 1e-5, "the core stands a skin off the face itself, not off the frame box: %s" % ((p - on) @ n)
    touched = False
    for s in range(10):
        w.Update(STEP, CFG)
        touched = touched or _touching(w, 0, 1)
        assert touched or s < 1, "no manifold against the obstacle within two steps"
        p = np.array([w.bodies[1]["pos"]["x"], w.bodies[1]["pos"]["y"]], dtype=np.float64)
        assert (p - on) @ n > 0.0, "step %d: the body is behind the face: %s" % (s, p)


# ---- 3. it does nothing where nothing is fast -------------------------------------------------------------------------------------------
def _pile(continuous):
    """A static tray (a floor and two posts) and 60 bodies of the four kinds in turn, 10 x 6, dropped from a little above each other.
    The bodies' inradii are 12.5 to 14: at factor 0.8 the cores stay 2.5 to 2.8 inside the outlines, clear of the 2 units a resting
    body may lie inside what it rests on (include/phyx_amd.h CONTINUOUS BODIES, resting bodies)."""
    w = phyx_amd.World(0, gravity=-200.0)
    w.add_bodies(np.array([[0.0, -10.0, 0.0, 350.0, 10.0], [-310.0, 60.0, 0.0, 10.0, 60.0], [310.0, 60.0, 0.0, 10.0, 60.0]], dtype=F))
    w.set_inverse_masses([0, 1, 2], np.zeros((3, 2), dtype=F))
    hexagon = ps.regular(6, 15.0)
    for row in range(6):
        for col in range(10):
            k = row * 10 + col
            x, y, a = -247.5 + 55.0 * col + 7.5 * (row % 2), 14.5 + 29.0 * row, 0.05 * ((k % 5) - 2)
            if k % 4 == 0:
                w.add_bodies(np.array([[x, y, a, 15.0, 12.5]], dtype=F))
            elif k % 4 == 1:
                w.add_circles(np.array([[x, y, a, 14.0]], dtype=F))
            elif k % 4 == 2:
                w.add_capsules(np.array([[x, y, a, 20.0, 12.5]], dtype=F))
            else:
                w.add_polygons(np.array([[x, y, a]], dtype=F), _verts(hexagon))
    if continuous:
        w.set_continuous(np.arange(3, 63, dtype=np.int32), factor=0.8)
    return w


def test_a_settling_pile_is_its_twin(built_lib):
    w, twin = _pile(True), _pile(False)
    assert (w.continuous()[3:] > 0).all() and not twin.continuous().any()
    for _ in range(120):
        w.Update(STEP, CFG)
        twin.Update(STEP, CFG)
    for a, b in zip(w.state(), twin.state()):
        assert a.tobytes() == b.tobytes()
    assert w.sweep_counts() == (120, 0) and not len(w.sweep_hits())
    assert twin.sweep_counts() == (0, 0)
    assert w.counts()[1] >= 50, "the pile has settled into contacts"


# ---- 4. no sticking -----------------------------------------------------------------------------------------------------------------------
def _pushed(continuous):
    w = phyx_amd.World(0, gravity=-200.0)
    w.add_bodies(np.array([[0.0, -2.0, 0.0, 400.0, 2.0], [-300.0, 1.95, 0.0, 2.0, 2.0]], dtype=F))
    w.set_inverse_masses([0], STATIC)
    if continuous:
        w.set_continuous([1])
    return w


def test_a_pushed_box_travels_as_far_as_its_twin(built_lib):
    w, twin = _pushed(True), _pushed(False)
    push = np.array([[100.0, 0.0, 0.0]], dtype=F)
    for _ in range(120):
        for x in (w, twin):
            x.add_accelerations([1], push)
            x.Update(STEP, CFG)
    assert w.bodies.tobytes() == twin.bodies.tobytes()
    assert w.bodies[1]["pos"]["x"] > -300.0 + 50.0, "the box went nowhere: %s" % w.bodies[1]["pos"]
    assert w.sweep_counts() == (120, 0)


def test_a_clamped_body_keeps_moving_sideways(built_lib):
    w, fly, n, on = _obstacle_world("wall", "marble", True)
    w.set_materials([0, 1], friction=0.0)
    w.Update(STEP, CFG)
    assert len(w.sweep_hits()) == 1
    ys = [float(w.bodies[1]["pos"]["y"])]
    for _ in range(6):
        w.add_accelerations([1], np.array([[0.0, 300.0, 0.0]], dtype=F))
        w.Update(STEP, CFG)
        ys.append(float(w.bodies[1]["pos"]["y"]))
    assert (np.diff(ys) > 0).all() and ys[-1] - ys[0] > 0.5, ys
    assert float(w.bodies[1]["pos"]["x"]) < -0.25


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------------------------
def _column_world():
    """A floor and six boxes of half size 1 above it, far from each other; bodies 2, 4 and 5 continuous with different radii."""
    w = phyx_amd.World(0, gravity=0.0)
    w.add_bodies(np.array([[0.0, -2.0, 0.0, 50.0, 1.0]] + [[-20.0 + 8.0 * k, 3.0, 0.0, 1.0, 1.0] for k in range(6)], dtype=F))
    w.set_inverse_masses([0], STATIC)
    w.set_continuous([2, 4, 5], [0.5, 0.25, 0.75])
    model = np.array([0, 0, 0.5, 0, 0.25, 0.75, 0], dtype=F)
    assert w.continuous().tobytes() == model.tobytes()
    return w, model


def test_the_column_through_spawn_and_removal(built_lib):
    w, model = _column_world()
    w.Update(DT, CFG)                                                       # (the column is on the device, with the list)
    w.add_bodies(np.array([[40.0, 3.0, 0.0, 1.0, 1.0], [48.0, 3.0, 0.0, 1.0, 1.0]], dtype=F))
    model = spec.spawn(model, 2)
    assert w.continuous().tobytes() == model.tobytes()
    w.set_continuous([7], [0.5])
    model[7] = 0.5
    keep = np.ones(9, dtype=bool)
    keep[[1, 4]] = False
    w.remove_bodies([1, 4])
    model = spec.remove(model, keep)
    assert w.continuous().tobytes() == model.tobytes() and model.tolist() == [0, 0.5, 0, 0.75, 0, 0.5, 0]
    # the list follows the new numbering: bodies 1, 3 and 5 are swept, and only they
    w.set_velocities([1, 2, 3, 5], np.tile(np.array([[0.0, -4.5 / DT, 0.0]], dtype=F), (4, 1)))
    w.Update(DT, CFG)
    assert w.sweep_hits()["body"].tolist() == [1, 3, 5] and (w.sweep_hits()["target"] == 0).all()
    assert w.bodies[2]["pos"]["y"] < -1.0, "the discrete body went through the floor"
    w.set_continuous([1, 3, 5], 0.0)
    passes = w.sweep_counts()[0]
    w.Update(DT, CFG)
    assert w.sweep_counts()[0] == passes and not len(w.sweep_hits()), "turning the last body discrete brings the passes to a halt"
    assert not w.continuous().any()


def test_the_column_through_set_state_and_snapshots(built_lib):
    w, model = _column_world()
    snap = w.save()
    fork = w.fork()
    assert fork.continuous().tobytes() == model.tobytes()
    w.set_state(*w.state())
    assert w.continuous().tobytes() == spec.set_state(7).tobytes()
    w.Update(DT, CFG)
    assert w.sweep_counts()[0] == 0
    w.load(snap)
    assert w.continuous().tobytes() == model.tobytes()
    # export and import: the column travels in the blob, and the loaded world sweeps like the saved one
    other = phyx_amd.World(0, gravity=0.0)
    other.load(Snapshot.from_bytes(snap.to_bytes()))
    assert other.continuous().tobytes() == model.tobytes()
    for x in (w, fork, other):
        x.set_velocities([2, 3], np.tile(np.array([[0.0, -4.5 / DT, 0.0]], dtype=F), (2, 1)))
        x.Update(DT, CFG)
    assert w.sweep_hits()["body"].tolist() == [2]
    assert w.sweep_hits().tobytes() == fork.sweep_hits().tobytes() == other.sweep_hits().tobytes()
    assert w.bodies.tobytes() == fork.bodies.tobytes() == other.bodies.tobytes()


def test_a_blob_without_the_column_is_what_it_was(built_lib):
    w, _ = _column_world()
    with_column = w.save().to_bytes()
    plain = phyx_amd.World(0, gravity=0.0)
    plain.add_bodies(np.array([[0.0, -2.0, 0.0, 50.0, 1.0]] + [[-20.0 + 8.0 * k, 3.0, 0.0, 1.0, 1.0] for k in range(6)], dtype=F))
    plain.set_inverse_masses([0], STATIC)
    blob = plain.save().to_bytes()
    assert len(with_column) == len(blob) + 16 * 7 and blob[32] & 8 == 0 and with_column[32] & 8 == 8 and blob[112:128] == bytes(16)
    assert with_column[:32] == blob[:32] and with_column[128:len(blob)] == blob[128:]
    back = phyx_amd.World(0, gravity=0.0)
    back.load(Snapshot.from_bytes(blob))
    assert not back.continuous().any() and back.bodies.tobytes() == plain.bodies.tobytes()
    back.Update(DT, CFG)
    assert back.sweep_counts() == (0, 0)
    broken = bytearray(with_column)
    broken[len(blob) + 3] = 0xBF                                            # body 0's core radius: 0 becomes -0.5
    with pytest.raises(PhxError) as e:
        Snapshot.from_bytes(bytes(broken))
    assert "core radius" in str(e.value)


def test_the_calls_refuse_what_the_header_says(built_lib):
    w, model = _column_world()
    for bodies, radii, text in (([7], [0.5], "body index 7 out of range"), ([2, 2], [0.5, 0.5], "body 2 appears twice"), ([1], [-0.5], "the core radius -0.5 of body 1 is not finite and >= 0"),
                                ([1], [float("nan")], "the core radius nan of body 1 is not finite and >= 0"), ([1], [1.0], "the core radius 1 of body 1 is not below its inradius 1"),
                                ([0], [1.5], "the core radius 1.5 of body 0 is not below its inradius 1")):
        with pytest.raises(PhxError) as e:
            w.set_continuous(bodies, radii)
        assert "phx_world_set_continuous: " + text in str(e.value), str(e.value)
        assert w.continuous().tobytes() == model.tobytes()
    # a later set_shapes / set_polygons that makes an rc too large is refused in the same words
    with pytest.raises(PhxError) as e:
        w.set_shapes([5], SHAPE_BOX, 2.0, 0.75)
    assert "phx_world_set_shapes: the core radius 0.75 of body 5 is not below its inradius 0.75" in str(e.value)
    with pytest.raises(PhxError) as e:
        w.set_polygons([2], [(-0.5, -0.5), (0.5, -0.5), (0.0, 0.5)])
    assert "phx_world_set_polygons: the core radius 0.5 of body 2 is not below its inradius" in str(e.value)
    assert (w.shapes()["kind"] == SHAPE_BOX).all() and w.continuous().tobytes() == model.tobytes()
    w.set_shapes([5], SHAPE_BOX, 2.0, 0.8)                                  # 0.75 < 0.8: accepted
    # mid-step
    w.PreSolve(DT)
    for call in (lambda: w.set_continuous([1], [0.5]), w.continuous, w.sweep_hits, w.sweep_counts):
        with pytest.raises(PhxError) as e:
            call()
        assert "between pre_solve / step_begin and finish_step / step_end" in str(e.value)
    w.FinishStep(DT, CFG)
    # sharded worlds
    with pytest.raises(PhxError) as e:
        w.set_shard(0, 2)
    assert "the world holds continuous bodies, which a sharded world does not carry" in str(e.value)
    plain = phyx_amd.World(0, gravity=0.0)
    plain.add_bodies(np.array([[0.0, 0.0, 0.0, 1.0, 1.0]], dtype=F))
    plain.set_shard(0, 2)
    with pytest.raises(PhxError) as e:
        plain.set_continuous([0], [0.5])
    assert "phx_world_set_continuous: a sharded world carries no continuous bodies" in str(e.value)
    # the hit list's capacity
    w.set_velocities([2, 4], np.tile(np.array([[0.0, -4.5 / DT, 0.0]], dtype=F), (2, 1)))
    w.Update(DT, CFG)
    total = C.c_int64(0)
    assert built_lib.phx_world_sweep_hits(w.h, None, 0, C.byref(total)) == -4 and total.value == 2
    assert "2 hits, room for 0" in built_lib.phx_last_error().decode()


def test_a_sleeper_is_a_target(built_lib):
    """A box asleep on the floor reads as static when the pass runs: a bullet is stopped at it."""
    w = phyx_amd.World(0, gravity=-200.0)
    w.add_bodies(np.array([[0.0, -2.0, 0.0, 50.0, 2.0], [0.0, 1.98, 0.0, 2.0, 2.0]], dtype=F))
    w.set_inverse_masses([0], STATIC)
    w.set_sleeping(1.0, 1.0, 0.1)
    for _ in range(60):
        w.Update(STEP, CFG)
    assert w.sleep_states()["asleep"].tolist() == [0, 1]
    w.add_circles(np.array([[-3.5, 2.0, 0.0, 0.25]], dtype=F))
    w.set_velocities([2], np.array([[300.0, 0.0, 0.0]], dtype=F))
    w.set_continuous([2])
    w.Update(STEP, CFG)
    hits = w.sweep_hits()
    assert len(hits) == 1 and hits[0]["body"] == 2 and hits[0]["target"] == 1, hits
    assert w.bodies[2]["pos"]["x"] < -2.0
