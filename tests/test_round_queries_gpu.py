"""Round queries on the device (include/phyx_amd.h, QUERIES: phx_world_query_circles / phx_world_cast_circles) held byte for byte to
tests/round_query_spec.py on both paths, after tests/test_shape_queries_gpu.py: the edges of the tree's levels on worlds of circles
and boxes in turn, the scan path's chunks, a stepped mixed pile queried before and inside a step, the directed corpus (the spec's
bytes, and through them the float64 judge's bounds), answers after set_poses and after a box became a circle, the capacity rule, the
device form, a sleeper, the host forms' refusals, no effect on the world, and examples/fit.c."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import fit_example
import listing_cases
import phyx_amd
import round_query_corpus as rc
import round_query_spec as spec
from phyx_amd import Configuration, DeviceBuffer, scenes
from phyx_amd.api import rigid_body_dtype, shape_dtype, shape_hit_dtype

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
F = np.float32
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)
PATHS = ("scan", "index")


@pytest.fixture(params=PATHS)
def path(request, monkeypatch):
    """PHX_QUERY_PATH for the worlds made in the test (read when a world is created)."""
    monkeypatch.setenv("PHX_QUERY_PATH", request.param)
    return request.param


def _kinds(w):
    return w.shapes()["kind"].astype(np.int32)


_spec = {}


def _want(what, bodies, kinds, queries, skip):
    """The specification's answer, computed once for the same bytes (the two paths ask the same question)."""
    key = (what, bodies.tobytes(), kinds.tobytes(), queries.tobytes(), skip)
    if key not in _spec:
        _spec[key] = (spec.query_circles if what == "circles" else spec.cast_circles)(bodies, kinds, queries, skip)
    return _spec[key]


def _random(bodies, rng, k):
    """k seeded circles and k casts over the extent of the bodies that can move (a ground is 20 000 wide), of all of them when none
    can, and over a 100-unit square when there are none."""
    moving = bodies[(bodies["inv_mass"] != 0) | (bodies["inv_inertia"] != 0)]
    bodies = moving if len(moving) else bodies
    n = len(bodies)
    lo = np.array([bodies["aabb_min"]["x"].min(), bodies["aabb_min"]["y"].min()], dtype=np.float64) if n else np.zeros(2)
    hi = np.array([bodies["aabb_max"]["x"].max(), bodies["aabb_max"]["y"].max()], dtype=np.float64) if n else np.full(2, 100.0)
    c = rng.uniform(lo - 10.0, hi + 10.0, size=(k, 2))
    circles = np.concatenate([c, rng.uniform(0.05, 12.0, (k, 1))], axis=1)
    ang = rng.uniform(0, 2 * np.pi, k)
    speed = rng.uniform(0.5, 3.0, k)
    casts = np.concatenate([circles[rng.permutation(k)], (np.cos(ang) * speed)[:, None], (np.sin(ang) * speed)[:, None], rng.uniform(0.0, 120.0, (k, 1))], axis=1)
    return circles.astype(F), casts.astype(F)


def _directed(bodies, b):
    """Casts aimed at body b that reach each kind of result when nothing else is in the way: a start inside, head on along the body's
    two axes, at a corner from both of its sides, and a cast that stops short."""
    pos = np.array([bodies["pos"]["x"][b], bodies["pos"]["y"][b]], dtype=np.float64)
    xv = np.array([bodies["xv"]["x"][b], bodies["xv"]["y"][b]], dtype=np.float64)
    yv = np.array([bodies["yv"]["x"][b], bodies["yv"]["y"][b]], dtype=np.float64)
    h = np.array([bodies["geom_size"]["x"][b], bodies["geom_size"]["y"][b]], dtype=np.float64)
    out = [[*pos, 0.5, 1.0, 0.5, 10.0],                                                      # inside
           [*(pos - 30.0 * xv), 0.5, *xv, 100.0], [*(pos - 30.0 * yv), 0.5, *yv, 100.0],     # the faces whose normals are -xv and -yv
           [*(pos - 30.0 * xv), 0.5, *xv, 5.0]]                                              # stops short
    corner = pos - h[0] * xv - h[1] * yv                                                     # the corner (-,-), from 0.3 rad off either face
    for al in (0.3, np.pi / 2 - 0.3):
        e = np.cos(al) * xv + np.sin(al) * yv
        out.append([*(corner - 30.0 * e), 0.5, *e, 100.0])
    return np.array(out, dtype=F)


def _check(w, circles, casts, what="", skips=(False, True)):
    bodies, kinds = w.bodies, _kinds(w)
    for skip in skips:
        off, hits = w.query_circles(circles, skip_static=skip)
        so, sh = _want("circles", bodies, kinds, circles, skip)
        assert off.tobytes() == so.tobytes() and hits.tobytes() == sh.tobytes(), "query_circles %s skip=%s" % (what, skip)
        got, want = w.cast_circles(casts, skip_static=skip), _want("casts", bodies, kinds, casts, skip)
        assert got.tobytes() == want.tobytes(), "cast_circles %s skip=%s: first differing cast %s" % (
            what, skip, next((i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()), None))
    return bodies, kinds


def _grid(n):
    """n rotated boxes on a grid (as test_shape_queries_gpu._grid): body 0 is the lower left corner."""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    return np.stack([(k % side) * 9.0, (k // side) * 9.0 + 20.0, k * 0.01, np.full(n, 4.0), np.full(n, 3.0)], axis=1).astype(F)


def _grid_world(n, round_=True):
    """The grid with every odd body a circle of radius 3.5 and every seventh body static; round_ = False: boxes only, and no call
    that would activate the shape column."""
    w = phyx_amd.World(0, gravity=G)
    if n:
        w.add_bodies(_grid(n))
        if round_ and n > 1:
            w.set_shapes(np.arange(1, n, 2), phyx_amd.SHAPE_CIRCLE, 3.5)
        fixed = np.arange(3, n, 7)
        if len(fixed):
            w.set_inverse_masses(fixed, np.zeros((len(fixed), 2), dtype=F))
    w.Update(DT, CFG)
    return w


def _level_queries(bodies, seed):
    n = len(bodies)
    circles, casts = _random(bodies, np.random.default_rng(seed), 40)
    far = [[-5000.0, -5000.0, 2.0]]                                     # far outside
    if n:
        lo = np.array([bodies["aabb_min"]["x"].min(), bodies["aabb_min"]["y"].min()], dtype=np.float64)
        hi = np.array([bodies["aabb_max"]["x"].max(), bodies["aabb_max"]["y"].max()], dtype=np.float64)
        far.append([*(0.5 * (lo + hi)), float(np.hypot(*(hi - lo)))])   # covers everything
        own = bodies[::max(1, n // 256)]                                # one per body (of the large grids: one per 16)
        far += [[x, y, 1.0] for x, y in zip(own["pos"]["x"], own["pos"]["y"])]
        casts = np.concatenate([casts, _directed(bodies, 0), [[-5000.0, -5000.0, 2.0, -1.0, 0.0, 100.0]]])
        if n > 1:                                                       # body 1, a circle of the bottom row, from below
            casts = np.concatenate([casts, [[float(bodies["pos"]["x"][1]), float(bodies["pos"]["y"][1]) - 30.0, 0.5, 0.0, 1.0, 100.0]]])
    return np.concatenate([circles, np.array(far, dtype=F)]).astype(F), casts.astype(F)


@pytest.mark.parametrize("n", (0, 1, 64, 65, 4096, 4097))
def test_level_edges(built_lib, path, n):
    """Worlds at the edges of the tree's levels, circles and boxes in turn: 40 random circles and casts, a circle far outside, one that
    covers everything, one per body, and (with bodies) the directed casts at body 0, which nothing hides from below and from the left,
    and one from below at body 1, a circle;
    with and without PHX_QUERY_SKIP_STATIC.  The spec's own answers show every kind of result a box gives."""
    w = _grid_world(n)
    circles, casts = _level_queries(w.bodies, n)
    bodies, kinds = _check(w, circles, casts, what="n=%d" % n)
    assert kinds.tolist() == [i % 2 for i in range(n)]
    detail = []
    spec.cast_circles(bodies, kinds, casts, detail=detail)
    assert set(detail) >= ({None, -1, (0, "x"), (1, "y"), 2} | ({6} if n > 1 else set()) if n else {None}), detail
    off, hits = _want("circles", bodies, kinds, circles, False)
    assert (off[-1] > 0) == (n > 0) and (n == 0 or (off[42] - off[41] == n and off[41] == off[40]))
    off, hits = w.query_circles(np.zeros((0, 3), dtype=F))
    assert off.tolist() == [0] and len(hits) == 0 and len(w.cast_circles(np.zeros((0, 6), dtype=F))) == 0


def test_a_world_without_a_shape_column(built_lib, path):
    """The 65-body grid as boxes only: no set_shapes call, the kinds' column was never made, and the answers are the spec's for boxes."""
    w = _grid_world(65, round_=False)
    circles, casts = _level_queries(w.bodies, 65)
    bodies = w.bodies
    for skip in (False, True):
        off, hits = w.query_circles(circles, skip_static=skip)
        so, sh = spec.query_circles(bodies, None, circles, skip)
        assert off.tobytes() == so.tobytes() and hits.tobytes() == sh.tobytes() and so[-1] > 65
        assert w.cast_circles(casts, skip_static=skip).tobytes() == spec.cast_circles(bodies, None, casts, skip).tobytes()
    assert not _kinds(w).any()


def _mixed(scene, steps):
    """The scene with every other body that can move a circle of its smaller half extent, stepped."""
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scene)
    b = w.bodies
    moving = np.flatnonzero((b["inv_mass"] != 0) | (b["inv_inertia"] != 0))[::2].astype(np.int32)
    radii = np.minimum(b["geom_size"]["x"], b["geom_size"]["y"])[moving].astype(F)
    w.set_shapes(moving, phyx_amd.SHAPE_CIRCLE, radii)
    w.set_inverse_masses(moving, phyx_amd.circle_inverse_masses(radii))
    for _ in range(steps):
        w.Update(DT, CFG)
    return w


@pytest.mark.parametrize("count", (65, 129))
def test_scan_chunks(built_lib, monkeypatch, count):
    """PHX_QUERY_SCAN_CHUNK=64 splits the scan path's (query, body block) table: the bytes of the unchunked result."""
    monkeypatch.setenv("PHX_QUERY_PATH", "scan")
    got = {}
    for chunk in (None, "64"):
        if chunk:
            monkeypatch.setenv("PHX_QUERY_SCAN_CHUNK", chunk)
        w = _mixed(scenes.falling(299, width=80.0, ymax=260.0), 3)
        assert w.counts()[0] == 300
        circles, _ = _random(w.bodies, np.random.default_rng(count), count)
        got[chunk] = [w.query_circles(circles, skip_static=skip) for skip in (False, True)]
        if chunk:
            for skip in (False, True):
                so, sh = spec.query_circles(w.bodies, _kinds(w), circles, skip)
                assert got[chunk][skip][0].tobytes() == so.tobytes() and got[chunk][skip][1].tobytes() == sh.tobytes()
    for a, b in zip(got[None], got["64"]):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0][-1] > 0


def test_stepped_scene(built_lib, path):
    """A mixed pile of boxes and circles after 30 steps (arbitrary frames): random queries and queries built from the bodies' own
    records: a circle at a body's position (it hits that body and what it rests on), a cast from a body's position (t = 0) and one from
    above it; before pre_solve, and between pre_solve and finish_step (the geometry before IntegratePosition)."""
    w = _mixed(scenes.tilted(200), 30)
    assert 190 <= w.counts()[0] <= 210 and 80 <= _kinds(w).sum() <= 110
    rng = np.random.default_rng(30)
    for stage in ("before pre_solve", "between pre_solve and finish_step"):
        bodies = w.bodies
        circles, casts = _random(bodies, rng, 100)
        pick = rng.integers(0, len(bodies), 50)
        pos = np.stack([bodies["pos"]["x"], bodies["pos"]["y"]], axis=1)[pick].astype(F)
        own = np.concatenate([pos, np.full((50, 1), 0.25, dtype=F)], axis=1)
        circles = np.concatenate([circles, own])
        casts = np.concatenate([casts,
                                np.concatenate([own, np.tile([0.0, -1.0, 50.0], (50, 1))], axis=1),
                                np.concatenate([pos + F(40.0) * np.array([0.0, 1.0], dtype=F), np.full((50, 1), 2.0), np.tile([0.0, -1.0, 100.0], (50, 1))], axis=1)]).astype(F)
        bodies, kinds = _check(w, circles.astype(F), casts, what=stage)
        off, _ = _want("circles", bodies, kinds, circles.astype(F), False)
        assert (np.diff(off)[100:] >= 1).all()                          # every body holds its own position
        assert (_want("casts", bodies, kinds, casts, False)["t"][100:150] == 0).all()
        if stage == "before pre_solve":
            w.PreSolve(DT)
    w.FinishStep(DT, CFG)


@pytest.mark.parametrize("name", [c.name for c in rc.cases()])
def test_corpus_queries_equal_the_spec_and_meet_the_judge(monkeypatch, name):
    """A world built from the corpus case's bodies (no step), on both paths: cast_circles and query_circles are byte-equal to
    round_query_spec, and the device's own answers meet the float64 judge by the bounds and the excused share of
    test_round_queries_cpu.test_spec_against_the_float64_judge (a kernel that drifted from the spec would still be held to the truth;
    equal bytes are judged once)."""
    c = rc.case(name)
    for path in PATHS:
        monkeypatch.setenv("PHX_QUERY_PATH", path)
        w = rc.world(c.bodies, c.kinds)
        bodies, kinds = w.bodies, _kinds(w)
        assert kinds.tolist() == c.kinds.tolist()
        for casts in (c.casts, c.near_casts):
            if not len(casts):
                continue
            got, want = w.cast_circles(casts), _want("casts", bodies, kinds, casts, False)
            assert got.tobytes() == want.tobytes(), "%s %s: casts %s" % (name, path, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[:8])
            near, worst = rc.judged("casts", rc.judge_casts, bodies, kinds, casts, got)
            if casts is c.casts:
                print("%s %s: worst in u: %s" % (name, path, rc.table(worst)))
                assert near.mean() <= rc.CAP
                rc.assert_bounds(worst, "%s %s" % (name, path))
        for circles in (c.circles, c.near_circles):
            if not len(circles):
                continue
            off, hits = w.query_circles(circles)
            so, sh = _want("circles", bodies, kinds, circles, False)
            assert off.tobytes() == so.tobytes() and hits.tobytes() == sh.tobytes(), "%s %s: circles" % (name, path)
            near = rc.judged("circles", lambda b, k, q, o: rc.judge_circles(b, k, q, o, hits), bodies, kinds, circles, off)
            assert circles is c.near_circles or near.mean() <= rc.CAP
        if name == "a row of discs from 3000":
            assert w.cast_circles(c.casts)["body"].tolist() == [3, 2, -1, 3, 2, -1, 3, 2, -1, 1, 2, -1]
        if c.kinds.all() or not len(c.casts):
            continue
        keep = np.flatnonzero(c.kinds == rc.BOX)                        # the case's boxes alone: a world without a shape column
        w = rc.world(c.bodies[keep], c.kinds[keep])
        assert w.cast_circles(c.casts[:64]).tobytes() == spec.cast_circles(w.bodies, None, c.casts[:64]).tobytes(), "%s %s: boxes only" % (name, path)


def test_staleness(built_lib, path):
    """Query, change, query again: every answer is the spec of the world as it is then."""
    rng = np.random.default_rng(5)
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scenes.piles(3, 50, ymax=220.0))

    def check(what):
        circles, casts = _random(w.bodies, rng, 32)
        _check(w, circles, casts, what=what, skips=(False,))

    check("host-staged, before the first step")
    w.Update(DT, CFG)
    check("after a step")
    n = w.counts()[0]
    idx = rng.choice(n, 20, replace=False)
    w.set_poses(idx, np.stack([rng.uniform(-300, 300, 20), rng.uniform(0, 400, 20), rng.uniform(0, 6, 20)], axis=1).astype(F))
    check("after set_poses")
    b = w.bodies[idx]
    own = np.stack([b["pos"]["x"], b["pos"]["y"], np.full(20, 0.25)], axis=1).astype(F)
    off, hits = w.query_circles(own)
    assert all(i in hits[off[k]:off[k + 1]] for k, i in enumerate(idx))                       # the new poses are what the queries see
    # a box becomes a circle: a query circle in its frame square's corner, clear of the disc, saw the box and no longer sees the circle
    one = int(idx[0])
    b = w.bodies[one]
    r = float(min(b["geom_size"]["x"], b["geom_size"]["y"]))
    w.set_shapes([one], phyx_amd.SHAPE_BOX, r, r)
    check("after set_shapes made a square")
    b = w.bodies[one]
    xv, yv = np.array([b["xv"]["x"], b["xv"]["y"]], dtype=np.float64), np.array([b["yv"]["x"], b["yv"]["y"]], dtype=np.float64)
    at = np.array([b["pos"]["x"], b["pos"]["y"]], dtype=np.float64) + 0.95 * r * (xv + yv)
    corner = np.array([[at[0], at[1], 0.01 * r]], dtype=F)
    off, hits = w.query_circles(corner)
    assert one in hits
    w.set_shapes([one], phyx_amd.SHAPE_CIRCLE, r)
    off, hits = w.query_circles(corner)
    assert one not in hits and _kinds(w)[one] == 1
    check("after set_shapes turned a box into a circle")
    w.Update(DT, CFG)
    check("after another step")


def test_capacity(built_lib, path):
    w = _mixed(scenes.wall(14, 12), 3)
    bodies, kinds = w.bodies, _kinds(w)
    circles, _ = _random(bodies, np.random.default_rng(8), 30)
    so, sh = spec.query_circles(bodies, kinds, circles)
    total = int(so[-1])
    assert total > 2
    offsets, out, t = np.zeros(31, dtype=np.int32), np.zeros(total, dtype=np.int32), C.c_int64(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert w.L.phx_world_query_circles(w.h, vp(circles), 30, 0, vp(offsets), vp(out), total - 1, C.byref(t)) == -4
    assert t.value == total and offsets.tobytes() == so.tobytes()
    assert w.L.phx_world_query_circles(w.h, vp(circles), 30, 0, vp(offsets), vp(out), int(t.value), C.byref(t)) == 0
    assert out.tobytes() == sh.tobytes() and offsets.tobytes() == so.tobytes()
    n = len(bodies)
    off, hits = w.query_circles(np.tile([0.0, 50.0, 5000.0], (8, 1)))      # (the wrapper's retry: 8 n > 1024 hits)
    assert 8 * n > 1024 and off.tolist() == [n * k for k in range(9)] and hits.tolist() == list(range(n)) * 8


def test_listing_protocol(built_lib, path):
    """phx_world_query_circles with hit_cap one short and exact, and circles that count no hit at all, on both paths."""
    w = listing_cases.world()
    bodies = w.bodies
    circles = np.array([[0.0, 100.0, 2000.0], [5000.0, 5000.0, 2.0], [0.0, 20.0, 4.0]], dtype=F)      # everything, nothing, a few boxes
    so, sh = spec.query_circles(bodies, None, circles)
    assert np.diff(so)[:2].tolist() == [len(bodies), 0] and so[3] - so[2] >= 1
    listing_cases.one_short(w, "phx_world_query_circles", "hits", circles, so, sh)
    listing_cases.counted_none(w, "phx_world_query_circles", np.tile(circles[1], (3, 1)))


def test_device_form(built_lib, path):
    w = _mixed(scenes.wall(14, 12), 3)
    _, casts = _random(w.bodies, np.random.default_rng(4), 64)
    ok = casts[0].copy()
    bad = np.tile(ok, (7, 1))
    bad[0, 3:5] = 0.0                                                  # d == (0, 0)
    bad[1, 5] = -1.0                                                   # max_t < 0
    bad[2, 3] = np.nan
    bad[3, 5] = np.inf
    bad[4, 2] = 0.0                                                    # r == 0
    bad[5, 2] = -2.0
    bad[6, 0] = -np.inf
    casts = np.concatenate([casts, bad]).astype(F)
    dc, dh = DeviceBuffer(casts.nbytes), DeviceBuffer(16 * len(casts))
    dc.from_host(casts)
    bodies, kinds = w.bodies, _kinds(w)
    for skip in (False, True):
        w.cast_circles_device(dc.address(), len(casts), dh.address(), skip_static=skip)
        w.sync()
        hit = dh.to_host().view(shape_hit_dtype)
        assert hit.tobytes() == spec.cast_circles(bodies, kinds, casts, skip).tobytes()
        assert hit[:-7].tobytes() == w.cast_circles(casts[:-7], skip_static=skip).tobytes()
        assert hit[-7:].tobytes() == spec.cast_circles(bodies[:0], None, bad).tobytes()      # body -1, every other field 0
    assert (hit["body"][:-7] >= 0).any()
    w.cast_circles_device(dc.address(), 0, dh.address())
    assert w.L.phx_world_cast_circles_device(w.h, None, 1, 0, None) == -1
    assert w.L.phx_world_cast_circles_device(w.h, dc.address(), 1, 2, dh.address()) == -1      # (flags)


def test_a_sleeping_body_is_not_static(built_lib, path):
    """Three columns of four boxes asleep on the ground: with PHX_QUERY_SKIP_STATIC the round queries still find them, as a world whose
    records carry the sleepers' own inverse masses would, and never the ground."""
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scenes.stack(3, 4))
    w.set_sleeping(20.0, 5.0, 3 * DT)
    for _ in range(30):                                                 # (calm from the first step: a few steps)
        w.Update(DT, CFG)
        if w.sleep_states()["asleep"][1:].all():
            break
    own = w.sleep_states()
    assert own["asleep"][1:].all() and not own["asleep"][0]
    bodies = w.bodies
    assert not bodies["inv_mass"][1:].any()                             # (the records show a sleeper as the step sees it)
    awake = bodies.copy()
    awake["inv_mass"], awake["inv_inertia"] = own["inv_mass"], own["inv_inertia"]
    circles, casts = _random(awake, np.random.default_rng(2), 24)
    casts = np.concatenate([casts, [[float(bodies["pos"]["x"][5]), 500.0, 2.0, 0.0, -1.0, 1000.0]]]).astype(F)
    off, hits = w.query_circles(circles, skip_static=True)
    so, sh = spec.query_circles(awake, None, circles, True)
    assert off.tobytes() == so.tobytes() and hits.tobytes() == sh.tobytes() and len(sh) and 0 not in sh
    got = w.cast_circles(casts, skip_static=True)
    assert got.tobytes() == spec.cast_circles(awake, None, casts, True).tobytes()
    assert got["body"][-1] == 8                                         # the top of column 1, asleep
    assert w.sleep_states()["asleep"][1:].all()                         # a query names no body: nobody woke


def test_queries_change_nothing(built_lib, path):
    """A world answering round queries between every step stays byte-equal to a twin that makes none, keeps its cached schedule, and
    builds the query index only when the geometry changed."""
    rng = np.random.default_rng(9)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)
    a, b = phyx_amd.World(0, gravity=0.0), phyx_amd.World(0, gravity=0.0)
    a.add_scene(scenes.stack(6, 10)); b.add_scene(scenes.stack(6, 10))
    a.query_circles([[0.0, 20.0, 3.0]])                                # (before the first step: host-staged bodies go up)
    for s in range(20):
        circles, casts = _random(b.bodies, rng, 16)                    # (from the twin: a makes nothing but the queries)
        builds = a.query_index()
        a.query_circles(circles); a.cast_circles(casts, skip_static=True); a.query_circles(circles, skip_static=True)
        assert a.query_index() == builds, "step %d: the geometry did not change" % s
        a.Update(DT, cfg)
        b.Update(DT, cfg)
        assert a.solver.stats().recoloured == b.solver.stats().recoloured, "step %d" % s
    assert a.build_counts() == b.build_counts()
    for x, y in zip(a.state(), b.state()):
        assert x.tobytes() == y.tobytes()
    assert a.solver.stats().recoloured == 0


def test_host_forms_refuse_bad_input(built_lib):
    """PHX_ERR_INVALID before anything is queued, one rule at a time, phx_last_error naming the call; count == 0 is valid."""
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scenes.stack(2, 3))
    w.Update(DT, CFG)
    L = w.L
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    good = np.array([0.0, 60.0, 2.0, 0.0, -1.0, 100.0], dtype=F)
    offsets, hits, t = np.zeros(2, dtype=np.int32), np.zeros(16, dtype=np.int32), C.c_int64(0)
    out = np.zeros(1, dtype=shape_hit_dtype)
    assert L.phx_world_query_circles(w.h, vp(np.array([0.0, 20.0, 2.0], dtype=F)), 1, 0, vp(offsets), vp(hits), 16, C.byref(t)) == 0 and t.value >= 1
    assert L.phx_world_cast_circles(w.h, vp(good), 1, 0, vp(out)) == 0 and out["body"][0] >= 0
    for col, value in ((0, np.nan), (1, np.inf), (2, 0.0), (2, -1.0), (2, np.nan)):
        q = good.copy(); q[col] = value
        assert L.phx_world_query_circles(w.h, vp(q), 1, 0, vp(offsets), vp(hits), 16, C.byref(t)) == -1, (col, value)
        assert L.phx_last_error().startswith(b"phx_world_query_circles: ")
        assert L.phx_world_cast_circles(w.h, vp(q), 1, 0, vp(out)) == -1, (col, value)
        assert L.phx_last_error().startswith(b"phx_world_cast_circles: ")
    for cols, value in (((5,), -1.0), ((5,), np.inf), ((3,), np.nan), ((3, 4), 0.0), ((3, 4), -0.0)):
        q = good.copy(); q[list(cols)] = value
        assert L.phx_world_cast_circles(w.h, vp(q), 1, 0, vp(out)) == -1, (cols, value)
        assert L.phx_last_error().startswith(b"phx_world_cast_circles: ")
    assert L.phx_world_query_circles(w.h, vp(good), 1, 2, vp(offsets), vp(hits), 16, C.byref(t)) == -1      # (flags)
    assert L.phx_world_query_circles(w.h, vp(good), -1, 0, vp(offsets), vp(hits), 16, C.byref(t)) == -1
    assert L.phx_world_query_circles(w.h, vp(good), 1, 0, None, vp(hits), 16, C.byref(t)) == -1
    assert L.phx_world_cast_circles(w.h, vp(good), 1, 0, None) == -1
    assert L.phx_world_cast_circles(w.h, None, 0, 0, None) == 0
    with pytest.raises(ValueError):
        w.cast_circles([[0.0, 60.0, 2.0, 0.0, 0.0, 1.0]])


def test_fit_example_runs_and_its_drop_is_the_specs(tmp_path, built_lib):
    """The marble emitter that looks first: the program queries the slot again after each spawn and fails if anything but the new
    marble is there; it must have spawned, and must have been refused while a marble was still in the slot.  The drop it prints is the
    specification's cast on the records it saw."""
    exe, dump = fit_example.build(tmp_path), str(tmp_path / "world.bin")
    r = subprocess.run([exe, "300", dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spawned into an occupied slot" not in r.stderr
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("fit:"))
    spawned, refused = int(line.split()[1]), int(line.split()[4])
    assert spawned >= 5 and refused >= 5 and spawned + refused == 300
    m = re.search(r"touches body (-?\d+) after t = (\S+), normal \((\S+), (\S+)\)", r.stdout)
    assert m, r.stdout
    raw = open(dump, "rb").read()
    nb = int(np.frombuffer(raw, dtype=np.int32, count=1)[0])
    assert nb == spawned + 5 and len(raw) == 4 + nb * (rigid_body_dtype.itemsize + shape_dtype.itemsize)
    bodies = np.frombuffer(raw, dtype=rigid_body_dtype, count=nb, offset=4)
    kinds = np.frombuffer(raw, dtype=shape_dtype, count=nb, offset=4 + nb * rigid_body_dtype.itemsize)["kind"].astype(np.int32)
    assert kinds.tolist() == [0] * 5 + [1] * spawned
    want = spec.cast_circles(bodies, kinds, [[0.0, 200.0, 3.0, 0.0, -1.0, 1000.0]])[0]
    assert want["body"] >= 0
    assert int(m.group(1)) == want["body"] and F(float(m.group(2))) == want["t"]
    assert (F(float(m.group(3))), F(float(m.group(4)))) == tuple(want["normal"])
