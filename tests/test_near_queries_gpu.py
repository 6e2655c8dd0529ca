"""Nearest-body queries on the device (include/phyx_amd.h, QUERIES: phx_world_query_nearest) held byte for byte to tests/near_spec.py on
both paths, after tests/test_round_queries_gpu.py: the edges of the tree's levels on a world of all four kinds at every max_dist, a
world without a shape column, the scan path's chunks, a stepped mixed pile queried before and inside a step, the directed corpus
(the spec's bytes, and the device's own answers held to the float64 judge), answers after set_poses, set_shapes and set_polygons, the
device form, a sleeper, no effect on the world, and the host form's refusals."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import near_corpus as nc
import near_spec as spec
import phyx_amd
import polygon_spec as ps
import reach_example
from phyx_amd import Configuration, DeviceBuffer, scenes
from phyx_amd.api import near_hit_dtype, rigid_body_dtype, shape_dtype

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = -200.0
F = np.float32
FLT_MAX = nc.FLT_MAX
MAX_DISTS = (0.0, 2.0, 50.0, FLT_MAX)
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)
PATHS = ("scan", "index")
PENTAGON = np.asarray(ps.regular(5, 3.5, 0.4)["v"])[:5]


@pytest.fixture(params=PATHS)
def path(request, monkeypatch):
    """PHX_QUERY_PATH for the worlds made in the test (read when a world is created)."""
    monkeypatch.setenv("PHX_QUERY_PATH", request.param)
    return request.param


def _kinds(w):
    return w.shapes()["kind"].astype(np.int32)


def _polys(w, kinds):
    return list(w.polygons()) if (kinds == phyx_amd.SHAPE_POLYGON).any() else [None] * len(kinds)


_spec = {}


def _want(bodies, kinds, polys, queries, skip):
    """The specification's answer, computed once for the same bytes (the two paths ask the same question)."""
    key = (bodies.tobytes(), kinds.tobytes(), b"".join(p.tobytes() for p in polys if p is not None), queries.tobytes(), skip)
    if key not in _spec:
        _spec[key] = spec.query_nearest(bodies, kinds, polys, queries, skip)
    return _spec[key]


def _random(bodies, rng, k):
    """k seeded queries over the extent of the bodies that can move (of all of them when none can, a 100-unit square when there are
    none), 10 units beyond it each way, max_dist cycling through 0, 2, 50 and FLT_MAX."""
    moving = bodies[(bodies["inv_mass"] != 0) | (bodies["inv_inertia"] != 0)]
    bodies = moving if len(moving) else bodies
    n = len(bodies)
    lo = np.array([bodies["aabb_min"]["x"].min(), bodies["aabb_min"]["y"].min()], dtype=np.float64) if n else np.zeros(2)
    hi = np.array([bodies["aabb_max"]["x"].max(), bodies["aabb_max"]["y"].max()], dtype=np.float64) if n else np.full(2, 100.0)
    p = rng.uniform(lo - 10.0, hi + 10.0, size=(k, 2))
    return np.concatenate([p, np.resize(MAX_DISTS, k)[:, None]], axis=1).astype(F)


def _check(w, queries, what="", skips=(False, True), polys=None):
    """(polys: the world's polygons where the caller has them; inside a step phx_world_get_polygons is refused)"""
    bodies, kinds = w.bodies, _kinds(w)
    polys = _polys(w, kinds) if polys is None else polys
    for skip in skips:
        got, want = w.query_nearest(queries, skip_static=skip), _want(bodies, kinds, polys, queries, skip)
        assert got.tobytes() == want.tobytes(), "query_nearest %s skip=%s: first differing query %s" % (
            what, skip, next((i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()), None))
    return bodies, kinds, polys


def _grid(n):
    """n rotated boxes on a grid (as test_round_queries_gpu._grid): body 0 is the lower left corner."""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    return np.stack([(k % side) * 9.0, (k // side) * 9.0 + 20.0, k * 0.01, np.full(n, 4.0), np.full(n, 3.0)], axis=1).astype(F)


def _grid_world(n, shaped=True):
    """The grid with every odd body a circle of radius 3.5, every sixth body from 2 a capsule {4, 1.5}, every sixteenth from 4 a
    pentagon and every seventh from 3 static; shaped = False: boxes only, and no call that would activate a shape column."""
    w = phyx_amd.World(0, gravity=G)
    if n:
        w.add_bodies(_grid(n))
        if shaped and n > 1:
            w.set_shapes(np.arange(1, n, 2), phyx_amd.SHAPE_CIRCLE, 3.5)
        if shaped and n > 2:
            w.set_shapes(np.arange(2, n, 6), phyx_amd.SHAPE_CAPSULE, 4.0, 1.5)
        if shaped and n > 4:
            w.set_polygons(np.arange(4, n, 16), PENTAGON)
        fixed = np.arange(3, n, 7)
        if len(fixed):
            w.set_inverse_masses(fixed, np.zeros((len(fixed), 2), dtype=F))
    w.Update(DT, CFG)
    return w


def _level_queries(bodies, seed):
    n = len(bodies)
    queries = _random(bodies, np.random.default_rng(seed), 32)
    extra = [[-5000.0, -5000.0, m] for m in MAX_DISTS]                     # far outside: found under FLT_MAX alone
    if n:
        own = bodies[::max(1, n // 16)]                                     # at a body's position (inside it), and 5 units above it
        extra += [[x, y, m] for k, (x, y) in enumerate(zip(own["pos"]["x"], own["pos"]["y"])) for m in (MAX_DISTS[k % 4],)]
        extra += [[x, y + 5.0, MAX_DISTS[(k + 1) % 4]] for k, (x, y) in enumerate(zip(own["pos"]["x"], own["pos"]["y"]))]
    return np.concatenate([queries, np.array(extra, dtype=F)]).astype(F)


@pytest.mark.parametrize("n", (0, 1, 64, 65, 4096, 4097))
def test_level_edges(built_lib, path, n):
    """Worlds at the edges of the tree's levels, all four kinds: 32 random queries, a point far outside at every max_dist, and points at
    and above a sample of the bodies; max_dist 0, 2, 50 and FLT_MAX; with and without PHX_QUERY_SKIP_STATIC."""
    w = _grid_world(n)
    queries = _level_queries(w.bodies, n)
    bodies, kinds, polys = _check(w, queries, what="n=%d" % n)
    want_kinds = [0] * n
    for i in range(n):
        want_kinds[i] = 3 if (i >= 4 and (i - 4) % 16 == 0) else 2 if (i >= 2 and (i - 2) % 6 == 0) else i % 2
    assert kinds.tolist() == want_kinds
    want = _want(bodies, kinds, polys, queries, False)
    assert want["body"][32:35].tolist() == [-1] * 3 and (want["body"][35] >= 0) == (n > 0)      # FLT_MAX: anywhere
    if n >= 64:
        found = set(kinds[want["body"][want["body"] >= 0]].tolist())
        assert found >= {0, 1, 2} and (want["distance"] < 0).any() and (want["distance"] > 0).any()
    assert len(w.query_nearest(np.zeros((0, 3), dtype=F))) == 0


def test_a_world_without_a_shape_column(built_lib, path):
    """The 65-body grid as boxes only: no set_shapes call, the kinds' column was never made, and the answers are the spec's for boxes."""
    w = _grid_world(65, shaped=False)
    queries = _level_queries(w.bodies, 65)
    bodies = w.bodies
    for skip in (False, True):
        want = spec.query_nearest(bodies, None, [None] * 65, queries, skip)
        assert w.query_nearest(queries, skip_static=skip).tobytes() == want.tobytes() and (want["body"] >= 0).sum() > 10
    assert not _kinds(w).any()


def _mixed(scene, steps):
    """The scene with the bodies that can move turned, in turn, into circles, capsules, hexagons and left boxes; stepped."""
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scene)
    b = w.bodies
    moving = np.flatnonzero((b["inv_mass"] != 0) | (b["inv_inertia"] != 0)).astype(np.int32)
    small = np.minimum(b["geom_size"]["x"], b["geom_size"]["y"]).astype(F)
    large = np.maximum(b["geom_size"]["x"], b["geom_size"]["y"]).astype(F)
    discs, caps, gons = moving[0::4], moving[1::4], moving[2::4]
    w.set_shapes(discs, phyx_amd.SHAPE_CIRCLE, small[discs])
    w.set_inverse_masses(discs, phyx_amd.circle_inverse_masses(small[discs]))
    w.set_shapes(caps, phyx_amd.SHAPE_CAPSULE, large[caps], F(0.75) * small[caps])
    w.set_polygons(gons, [np.asarray(ps.regular(6, float(small[i]), 0.1)["v"])[:6] for i in gons])
    for _ in range(steps):
        w.Update(DT, CFG)
    return w


@pytest.mark.parametrize("count", (65, 129))
def test_scan_chunks(built_lib, monkeypatch, count):
    """PHX_QUERY_SCAN_CHUNK=64 splits the scan path's launches: the bytes of the unchunked result, and the spec's."""
    monkeypatch.setenv("PHX_QUERY_PATH", "scan")
    got = {}
    for chunk in (None, "64"):
        if chunk:
            monkeypatch.setenv("PHX_QUERY_SCAN_CHUNK", chunk)
        w = _mixed(scenes.falling(299, width=80.0, ymax=260.0), 3)
        assert w.counts()[0] == 300
        queries = _random(w.bodies, np.random.default_rng(count), count)
        got[chunk] = [w.query_nearest(queries, skip_static=skip) for skip in (False, True)]
        if chunk:
            _check(w, queries, what="chunk 64")
    for a, b in zip(got[None], got["64"]):
        assert a.tobytes() == b.tobytes() and (a["body"] >= 0).sum() > count // 4


def test_stepped_scene(built_lib, path):
    """A mixed pile of all four kinds after 30 steps (arbitrary frames): random queries and queries built from the bodies' own
    records (at a body's position: inside it; 40 above it, anywhere); before pre_solve, and between pre_solve and finish_step (the
    geometry before IntegratePosition)."""
    w = _mixed(scenes.tilted(200), 30)
    assert 190 <= w.counts()[0] <= 210 and set(_kinds(w).tolist()) == {0, 1, 2, 3}
    rng = np.random.default_rng(30)
    polys = _polys(w, _kinds(w))                                        # (a step moves no vertex; the getter is refused inside one)
    for stage in ("before pre_solve", "between pre_solve and finish_step"):
        bodies = w.bodies
        pick = rng.integers(0, len(bodies), 50)
        pos = np.stack([bodies["pos"]["x"], bodies["pos"]["y"]], axis=1)[pick].astype(F)
        own = np.concatenate([pos, np.full((50, 1), 1.0, dtype=F)], axis=1)
        above = np.concatenate([pos + F(40.0) * np.array([0.0, 1.0], dtype=F), np.full((50, 1), FLT_MAX, dtype=F)], axis=1)
        queries = np.concatenate([_random(bodies, rng, 100), own, above]).astype(F)
        bodies, kinds, _ = _check(w, queries, what=stage, polys=polys)
        want = _want(bodies, kinds, polys, queries, False)
        assert (want["distance"][100:150] < 0).all() and (want["body"][150:] >= 0).all()      # every body holds its own position
        if stage == "before pre_solve":
            w.PreSolve(DT)
    w.FinishStep(DT, CFG)


@pytest.mark.parametrize("name", [c.name for c in nc.cases()])
def test_corpus_queries_equal_the_spec_and_meet_the_judge(monkeypatch, name):
    """A world built from the corpus case's bodies (no step), on both paths: query_nearest is byte-equal to near_spec, and the device's
    own answers meet the float64 judge by the bounds and the excused share of test_near_queries_cpu (a kernel that drifted from the
    spec would still be held to the truth; equal bytes are judged once)."""
    c = nc.case(name)
    for path in PATHS:
        monkeypatch.setenv("PHX_QUERY_PATH", path)
        w = nc.world(c.bodies, c.kinds, c.polys)
        bodies, kinds = w.bodies, _kinds(w)
        polys = _polys(w, kinds)
        assert kinds.tolist() == c.kinds.tolist()
        for queries in (c.queries, c.near_queries):
            if not len(queries):
                continue
            got, want = w.query_nearest(queries), _want(bodies, kinds, polys, queries, False)
            assert got.tobytes() == want.tobytes(), "%s %s: queries %s" % (name, path, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[:8])
            pairs, worst = nc.judged("nearest", lambda b, k, q, o: nc.judge_near(b, k, polys, q, o), bodies, kinds, queries, got)
            nc.assert_bounds(worst, "%s %s" % (name, path))
            if queries is c.queries:
                print("%s %s: worst in u: %s" % (name, path, nc.table(worst)))
                assert pairs.mean() <= nc.CAP
        keep = np.flatnonzero(c.kinds == nc.BOX)                            # the case's boxes alone: a world without a shape column
        w = nc.world(c.bodies[keep], c.kinds[keep], [None] * len(keep))
        assert w.query_nearest(c.queries[:64]).tobytes() == spec.query_nearest(w.bodies, None, [None] * len(keep), c.queries[:64]).tobytes(), "%s %s: boxes only" % (name, path)


def test_staleness(built_lib, path):
    """Query, change, query again: every answer is the spec of the world as it is then."""
    rng = np.random.default_rng(5)
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scenes.piles(3, 50, ymax=220.0))

    def check(what):
        _check(w, _random(w.bodies, rng, 32), what=what, skips=(False,))

    check("host-staged, before the first step")
    w.Update(DT, CFG)
    check("after a step")
    n = w.counts()[0]
    idx = rng.choice(n, 20, replace=False)
    w.set_poses(idx, np.stack([rng.uniform(-300, 300, 20), rng.uniform(0, 400, 20), rng.uniform(0, 6, 20)], axis=1).astype(F))
    check("after set_poses")
    b = w.bodies[idx]
    own = np.stack([b["pos"]["x"], b["pos"]["y"], np.zeros(20)], axis=1).astype(F)
    got = w.query_nearest(own)
    assert (got["body"] >= 0).all() and (got["distance"] <= 0).all()          # the new poses are what the queries see (max_dist 0: inside)
    # a box becomes a circle: a point in its frame square's corner was inside the box and is outside the disc
    one = int(idx[0])
    r = float(min(w.bodies[one]["geom_size"]["x"], w.bodies[one]["geom_size"]["y"]))
    w.set_shapes([one], phyx_amd.SHAPE_BOX, r, r)
    check("after set_shapes made a square")
    b = w.bodies[one]
    xv, yv = np.array([b["xv"]["x"], b["xv"]["y"]], dtype=np.float64), np.array([b["yv"]["x"], b["yv"]["y"]], dtype=np.float64)
    at = np.array([b["pos"]["x"], b["pos"]["y"]], dtype=np.float64) + 0.95 * r * (xv + yv)
    corner = np.array([[at[0], at[1], 0.0]], dtype=F)
    assert one in w.query_nearest(corner)["body"]
    w.set_shapes([one], phyx_amd.SHAPE_CIRCLE, r)
    assert one not in w.query_nearest(corner)["body"] and _kinds(w)[one] == 1
    check("after set_shapes turned a box into a circle")
    tri = [(-0.9 * r, -0.9 * r), (0.9 * r, -0.9 * r), (0.0, 0.9 * r)]       # ... and a triangle, which leaves its frame box's upper corners free
    w.set_polygons([one], tri)
    corner[0, 2] = 0.05 * r
    assert one not in w.query_nearest(corner)["body"] and _kinds(w)[one] == 3
    check("after set_polygons turned it into a triangle")
    w.Update(DT, CFG)
    check("after another step")


def test_device_form(built_lib, path):
    w = _mixed(scenes.wall(14, 12), 3)
    queries = _random(w.bodies, np.random.default_rng(4), 64)
    bad = np.tile(queries[1], (5, 1))
    bad[0, 2] = -1.0                                                   # max_dist < 0
    bad[1, 2] = np.nan
    bad[2, 2] = np.inf
    bad[3, 0] = np.nan
    bad[4, 1] = -np.inf
    queries = np.concatenate([queries, bad]).astype(F)
    dq, dh = DeviceBuffer(queries.nbytes), DeviceBuffer(24 * len(queries))
    dq.from_host(queries)
    bodies, kinds = w.bodies, _kinds(w)
    polys = _polys(w, kinds)
    for skip in (False, True):
        w.query_nearest_device(dq.address(), len(queries), dh.address(), skip_static=skip)
        w.sync()
        hit = dh.to_host().view(near_hit_dtype)
        assert hit.tobytes() == spec.query_nearest(bodies, kinds, polys, queries, skip).tobytes()
        assert hit[:-5].tobytes() == w.query_nearest(queries[:-5], skip_static=skip).tobytes()
        assert hit[-5:].tobytes() == spec.query_nearest(bodies[:0], None, [], bad).tobytes()      # body -1, every other field 0
    assert (hit["body"][:-5] >= 0).any()
    w.query_nearest_device(dq.address(), 0, dh.address())
    assert w.L.phx_world_query_nearest_device(w.h, None, 1, 0, None) == -1
    assert w.L.phx_world_query_nearest_device(w.h, dq.address(), 1, 2, dh.address()) == -1      # (flags)


def test_a_sleeping_body_is_not_static(built_lib, path):
    """Three columns of four boxes asleep on the ground: with PHX_QUERY_SKIP_STATIC the nearest query still finds them, as a world
    whose records carry the sleepers' own inverse masses would, and never the ground."""
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
    queries = _random(awake, np.random.default_rng(2), 24)
    queries = np.concatenate([queries, [[float(bodies["pos"]["x"][5]), 500.0, FLT_MAX], [float(bodies["pos"]["x"][5]), -3.0, FLT_MAX]]]).astype(F)
    got = w.query_nearest(queries, skip_static=True)
    assert got.tobytes() == spec.query_nearest(awake, None, [None] * len(awake), queries, True).tobytes()
    assert got["body"][-2] == 8 and got["body"][-1] > 0                 # the top of column 1, asleep; below the ground's surface: still no ground
    assert w.query_nearest(queries[-1:])["body"][0] == 0                # ... which is the nearest without the flag
    assert w.sleep_states()["asleep"][1:].all()                         # a query names no body: nobody woke


def test_queries_change_nothing(built_lib, path):
    """A world answering nearest queries between every step stays byte-equal to a twin that makes none, keeps its cached schedule, and
    builds the query index only when the geometry changed."""
    rng = np.random.default_rng(9)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)
    a, b = phyx_amd.World(0, gravity=0.0), phyx_amd.World(0, gravity=0.0)
    a.add_scene(scenes.stack(6, 10)); b.add_scene(scenes.stack(6, 10))
    a.query_nearest([[0.0, 20.0, 3.0]])                                # (before the first step: host-staged bodies go up)
    for s in range(20):
        queries = _random(b.bodies, rng, 16)                           # (from the twin: a makes nothing but the queries)
        builds = a.query_index()
        a.query_nearest(queries); a.query_nearest(queries, skip_static=True)
        assert a.query_index() == builds, "step %d: the geometry did not change" % s
        a.Update(DT, cfg)
        b.Update(DT, cfg)
        assert a.solver.stats().recoloured == b.solver.stats().recoloured, "step %d" % s
    assert a.build_counts() == b.build_counts()
    for x, y in zip(a.state(), b.state()):
        assert x.tobytes() == y.tobytes()
    assert a.solver.stats().recoloured == 0


def test_host_form_refuses_bad_input(built_lib):
    """PHX_ERR_INVALID before anything is queued, one rule at a time, phx_last_error naming the call; count == 0 and max_dist == 0
    are valid."""
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scenes.stack(2, 3))
    w.Update(DT, CFG)
    L = w.L
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    good = np.array([0.0, 60.0, 100.0], dtype=F)
    out = np.zeros(1, dtype=near_hit_dtype)
    assert L.phx_world_query_nearest(w.h, vp(good), 1, 0, vp(out)) == 0 and out["body"][0] >= 0
    for col, value in ((0, np.nan), (1, np.inf), (2, -1.0), (2, np.nan), (2, np.inf), (2, -np.inf)):
        q = good.copy(); q[col] = value
        assert L.phx_world_query_nearest(w.h, vp(q), 1, 0, vp(out)) == -1, (col, value)
        assert L.phx_last_error().startswith(b"phx_world_query_nearest: ")
    q = good.copy(); q[2] = 0.0
    assert L.phx_world_query_nearest(w.h, vp(q), 1, 0, vp(out)) == 0 and out["body"][0] == -1
    assert L.phx_world_query_nearest(w.h, vp(good), 1, 2, vp(out)) == -1      # (flags)
    assert L.phx_world_query_nearest(w.h, vp(good), -1, 0, vp(out)) == -1
    assert L.phx_world_query_nearest(w.h, vp(good), 1, 0, None) == -1
    assert L.phx_world_query_nearest(w.h, None, 1, 0, vp(out)) == -1
    assert L.phx_world_query_nearest(w.h, None, 0, 0, None) == 0
    with pytest.raises(ValueError):
        w.query_nearest([[0.0, 60.0, -1.0]])
    empty = phyx_amd.World(0, gravity=G)
    assert empty.query_nearest([good])[0].tobytes() == spec.query_nearest(w.bodies[:0], None, [], [good])[0].tobytes()


def test_reach_example_runs_and_its_pick_is_the_specs(tmp_path, built_lib):
    """The tolerant pick: the program fails if a marble is inside the funnel without a contact, and must have picked something.  The
    pick it prints is the specification's nearest dynamic body within 2 units of the cursor on the records it saw."""
    exe, dump = reach_example.build(tmp_path), str(tmp_path / "world.bin")
    r = subprocess.run([exe, "360", dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "has no contact" not in r.stderr
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("reach:"))
    assert int(line.split()[1]) >= 5 and int(line.split()[3]) >= 1
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("second ")]) == 6
    m = re.search(r"reached body (-?\d+) at distance (\S+) from \((\S+), (\S+)\), surface point \((\S+), (\S+)\)", r.stdout)
    assert m, r.stdout
    raw = open(dump, "rb").read()
    nb = int(np.frombuffer(raw, dtype=np.int32, count=1)[0])
    assert len(raw) == 4 + nb * (rigid_body_dtype.itemsize + shape_dtype.itemsize)
    bodies = np.frombuffer(raw, dtype=rigid_body_dtype, count=nb, offset=4)
    kinds = np.frombuffer(raw, dtype=shape_dtype, count=nb, offset=4 + nb * rigid_body_dtype.itemsize)["kind"].astype(np.int32)
    assert kinds.tolist() == [0] * 5 + [1] * (nb - 5)
    query = [[float(m.group(3)), float(m.group(4)), 2.0]]
    want = spec.query_nearest(bodies, kinds, [None] * nb, query, skip_static=True)[0]
    assert want["body"] >= 5 and int(m.group(1)) == want["body"] and F(float(m.group(2))) == want["distance"]
    assert (F(float(m.group(5))), F(float(m.group(6)))) == tuple(want["point"])
    assert spec.query_nearest(bodies, kinds, [None] * nb, query)[0]["distance"] <= want["distance"]      # (the floor may be nearer: it is never grabbed)
