"""Queries on the device (include/phyx_amd.h, QUERIES) held byte for byte to tests/query_spec.py: seeded and boundary queries on four
scenes through the scan path, the index path and the automatic choice; answers after every kind of change (no stale index); no effect
on the world; the edges of the tree's levels and of the AABB buffer; the device forms; the cfg 2 world; examples/pick.c; the boxes of
the directed corpus (tests/query_corpus.py) held to the spec's bytes and to the float64 judge (tests/query_reference.py), and oriented
boxes and casts on a field moved out to 10^5."""
import os
import subprocess

import numpy as np
import pytest

import listing_cases
import phyx_amd
import query_corpus as qc
import query_spec as spec
import shape_query_spec
from phyx_amd import Configuration, DeviceBuffer, scenes
from phyx_amd.api import ray_hit_dtype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1.0 / 60.0
G = -200.0
F = np.float32
CFG = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)
PATHS = ("scan", "index", None)
SCENES = {"stack": lambda: scenes.stack(6, 30),
          "wall": lambda: scenes.wall(14, 12),
          "falling": lambda: scenes.falling(300, width=80.0, ymax=260.0),
          "piles": lambda: scenes.piles(3, 50, ymax=220.0)}


@pytest.fixture
def path(request, monkeypatch):
    """PHX_QUERY_PATH for the worlds made in the test (read when a world is created)."""
    if request.param is None:
        monkeypatch.delenv("PHX_QUERY_PATH", raising=False)
    else:
        monkeypatch.setenv("PHX_QUERY_PATH", request.param)
    return request.param


def _world(scene, gravity=G):
    w = phyx_amd.World(0, gravity=gravity)
    w.add_scene(scene)
    return w


def _queries(bodies, rng, k=48):
    """Seeded boxes, points and rays over the bodies' extent, plus queries that sit exactly on boundaries: points at AABB and box
    corners, rays aimed at corners and along AABB edges, boxes equal to a body's AABB."""
    n = len(bodies)
    lo = np.array([bodies["aabb_min"]["x"].min(), bodies["aabb_min"]["y"].min()], dtype=np.float64) if n else np.zeros(2)
    hi = np.array([bodies["aabb_max"]["x"].max(), bodies["aabb_max"]["y"].max()], dtype=np.float64) if n else np.ones(2)
    hi = np.minimum(hi, lo + 4000.0)                                    # (the ground is 20 000 wide: stay near the bodies)
    lo = np.maximum(lo, hi - 4000.0)
    pts = rng.uniform(lo, hi, size=(k, 2))
    c = rng.uniform(lo, hi, size=(k, 2))
    ext = rng.uniform(0.0, 60.0, size=(k, 2))
    boxes = np.concatenate([c - ext, c + ext], axis=1)
    ang = rng.uniform(0.0, 2.0 * np.pi, size=k)
    rays = np.stack([pts[:, 0], pts[:, 1], np.cos(ang) * rng.uniform(0.5, 3.0, k), np.sin(ang) * rng.uniform(0.5, 3.0, k), rng.uniform(0.0, 400.0, k)], axis=1)
    if n:
        pick = rng.integers(0, n, size=min(k, n))
        b = bodies[pick]
        amin = np.stack([b["aabb_min"]["x"], b["aabb_min"]["y"]], axis=1).astype(np.float64)
        amax = np.stack([b["aabb_max"]["x"], b["aabb_max"]["y"]], axis=1).astype(np.float64)
        pos = np.stack([b["pos"]["x"], b["pos"]["y"]], axis=1).astype(F)
        xv = np.stack([b["xv"]["x"], b["xv"]["y"]], axis=1).astype(F)
        yv = np.stack([b["yv"]["x"], b["yv"]["y"]], axis=1).astype(F)
        h = np.stack([b["geom_size"]["x"], b["geom_size"]["y"]], axis=1).astype(F)
        corner = pos + xv * h[:, :1] + yv * h[:, 1:]                   # a box corner (float32 arithmetic)
        pts = np.concatenate([pts, amin, amax, np.stack([amin[:, 0], amax[:, 1]], axis=1), corner, pos])
        boxes = np.concatenate([boxes, np.concatenate([amin, amax], axis=1)])
        src = corner + np.array([-37.0, -23.0], dtype=F)
        at_corner = np.concatenate([src, corner - src, np.full((len(src), 1), 2.0)], axis=1)
        along_edge = np.concatenate([amin - [50.0, 0.0], np.tile([1.0, 0.0], (len(amin), 1)), np.full((len(amin), 1), 500.0)], axis=1)
        down = np.concatenate([pos + [0.0, 100.0], np.tile([0.0, -1.0], (len(pos), 1)), np.full((len(pos), 1), 1000.0)], axis=1)
        rays = np.concatenate([rays, at_corner, along_edge, down])
    return boxes.astype(F), pts.astype(F), rays.astype(F)


def _check(w, rng, k=48, what=""):
    bodies = w.bodies
    boxes, pts, rays = _queries(bodies, rng, k)
    for skip in (False, True):
        off, hits = w.query_aabb(boxes, skip_static=skip)
        so, sh = spec.query_aabb(bodies, boxes, skip)
        assert off.tobytes() == so.tobytes() and hits.tobytes() == sh.tobytes(), "query_aabb %s skip=%s" % (what, skip)
        assert w.query_points(pts, skip_static=skip).tobytes() == spec.query_points(bodies, pts, skip).tobytes(), "query_points %s skip=%s" % (what, skip)
        got, want = w.raycast(rays, skip_static=skip), spec.raycast(bodies, rays, skip)
        assert got.tobytes() == want.tobytes(), "raycast %s skip=%s: first differing ray %s" % (
            what, skip, next((i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()), None))


@pytest.mark.parametrize("path", PATHS, indirect=True)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_exact_on_scenes(built_lib, scene, path):
    w = _world(SCENES[scene]())
    rng = np.random.default_rng(len(scene))
    for s in range(4):
        w.Update(DT, CFG)
    _check(w, rng, what="%s after 4 steps" % scene)


@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
def test_staleness(built_lib, path):
    """Query, change, query again: every answer is the spec of the world as it is then."""
    rng = np.random.default_rng(5)
    w = _world(scenes.piles(3, 50, ymax=220.0))
    _check(w, rng, what="host-staged, before the first step")
    w.Update(DT, CFG)
    _check(w, rng, what="after a step")
    w.Update(DT, CFG)
    _check(w, rng, what="after a second step")
    n = w.counts()[0]
    idx = rng.choice(n, 20, replace=False)
    poses = np.stack([rng.uniform(-300, 300, 20), rng.uniform(0, 400, 20), rng.uniform(0, 6, 20)], axis=1).astype(F)
    w.set_poses(idx, poses)
    _check(w, rng, what="after set_poses")
    w.add_bodies(np.array([[x, 150.0, 0.3, 6.0, 4.0] for x in np.linspace(-200, 200, 30)], dtype=F))
    _check(w, rng, what="after add_bodies")
    w.remove_bodies(rng.choice(w.counts()[0], 25, replace=False))
    _check(w, rng, what="after remove_bodies")
    w.set_inverse_masses(np.arange(1, 11), np.zeros((10, 2), dtype=F))
    _check(w, rng, what="after set_inverse_masses (SKIP_STATIC)")
    st = w.state()
    b = st[0].copy()
    b["pos"]["x"] += F(1.5)
    b["geom_pos"]["x"] += F(1.5)
    b["aabb_min"]["x"] += F(1.5)
    b["aabb_max"]["x"] += F(1.5)
    w.set_state(b, *st[1:])
    _check(w, rng, what="after set_state")
    w.Update(DT, CFG)
    w.PreSolve(DT)
    _check(w, rng, what="between pre_solve and finish_step")
    w.FinishStep(DT, CFG)
    _check(w, rng, what="after finish_step")


def test_index_is_cached_until_the_geometry_changes(built_lib, monkeypatch):
    monkeypatch.setenv("PHX_QUERY_PATH", "index")
    w = _world(scenes.stack(6, 30))
    w.Update(DT, CFG)
    pts = np.array([[0.0, 20.0], [5.0, 40.0]], dtype=F)
    w.query_points(pts)
    b0 = w.query_index()
    w.query_points(pts); w.raycast([[0, 400, 0, -1, 1000]]); w.query_aabb([[-50, 0, 50, 100]])
    assert w.query_index() == b0                                        # the same geometry: no rebuild
    w.add_accelerations([3], [[0.0, 10.0, 0.0]])
    w.set_velocities([4], [[1.0, 0.0, 0.0]])
    assert w.query_index() == b0                                        # (neither moves a body before the next step)
    w.Update(DT, CFG)
    assert w.query_index() == b0 + 1


@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
def test_queries_change_nothing(built_lib, path):
    """A world answering queries between every step stays byte-equal to a twin that makes none, and keeps its cached schedule."""
    rng = np.random.default_rng(9)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)
    a, b = _world(scenes.stack(6, 10), 0.0), _world(scenes.stack(6, 10), 0.0)
    a.query_points([[0.0, 20.0]])                                       # (before the first step: host-staged bodies go up)
    for s in range(20):
        boxes, pts, rays = _queries(b.bodies, rng, 16)                 # (from the twin: a makes nothing but the queries)
        a.query_aabb(boxes); a.query_points(pts, skip_static=True); a.raycast(rays)
        a.Update(DT, cfg)
        b.Update(DT, cfg)
        assert a.solver.stats().recoloured == b.solver.stats().recoloured, "step %d" % s
    assert a.build_counts() == b.build_counts()
    for x, y in zip(a.state(), b.state()):
        assert x.tobytes() == y.tobytes()
    assert a.solver.stats().recoloured == 0


@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
@pytest.mark.parametrize("n", (0, 1, 64, 65, 4096, 4097))
def test_level_edges(built_lib, path, n):
    w = phyx_amd.World(0, gravity=G)
    if n:
        side = int(np.ceil(np.sqrt(n)))
        k = np.arange(n)
        rows = np.stack([(k % side) * 9.0, (k // side) * 9.0 + 20.0, k * 0.01, np.full(n, 4.0), np.full(n, 3.0)], axis=1).astype(F)
        w.add_bodies(rows)
    w.Update(DT, CFG)
    _check(w, np.random.default_rng(n), k=40, what="n=%d" % n)
    off, hits = w.query_aabb(np.zeros((0, 4), dtype=F))
    assert off.tolist() == [0] and len(hits) == 0
    assert len(w.query_points(np.zeros((0, 2), dtype=F))) == 0 and len(w.raycast(np.zeros((0, 5), dtype=F))) == 0


def _cfg2(steps=30):
    w = _world(scenes.stack(1000, 200))
    for _ in range(steps):
        w.Update(DT, CFG)
    return w


def test_cfg2_world(built_lib, monkeypatch):
    """The cfg 2 world (200 001 bodies) after 30 steps: a few hundred queries on both paths against the spec; one box over the whole
    world (one segment of 200 001 hits, ascending); hit_cap one short gives PHX_ERR_CAPACITY with the total, then the exact result."""
    import ctypes as C
    rng = np.random.default_rng(2)
    for p in ("scan", "index"):
        monkeypatch.setenv("PHX_QUERY_PATH", p)
        w = _cfg2()
        bodies = w.bodies
        boxes, pts, rays = _queries(bodies, rng, 120)
        got = w.query_aabb(boxes)
        want = spec.query_aabb(bodies, boxes)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), p
        assert w.query_points(pts, skip_static=True).tobytes() == spec.query_points(bodies, pts, True).tobytes(), p
        assert w.raycast(rays).tobytes() == spec.raycast(bodies, rays).tobytes(), p
        n = len(bodies)
        every = np.array([[-1e30, -1e30, 1e30, 1e30]], dtype=F)
        off, hits = w.query_aabb(every)
        assert off.tolist() == [0, n] and hits.tolist() == list(range(n)), p
        two = np.array([[-1e30, -1e30, 1e30, 1e30], [-20, 0, 20, 40]], dtype=F)
        so, sh = spec.query_aabb(bodies, two)
        total = int(so[-1])
        offsets = np.zeros(3, dtype=np.int32)
        out = np.zeros(total, dtype=np.int32)
        t = C.c_int64(0)
        L = w.L
        vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        assert L.phx_world_query_aabb(w.h, vp(two), 2, 0, vp(offsets), vp(out), total - 1, C.byref(t)) == -4
        assert t.value == total and offsets.tobytes() == so.tobytes()
        assert L.phx_world_query_aabb(w.h, vp(two), 2, 0, vp(offsets), vp(out), total, C.byref(t)) == 0
        assert out.tobytes() == sh.tobytes() and offsets.tobytes() == so.tobytes()
        del w


@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
def test_device_forms(built_lib, path):
    rng = np.random.default_rng(4)
    w = _world(scenes.wall(14, 12))
    for _ in range(3):
        w.Update(DT, CFG)
    _, pts, rays = _queries(w.bodies, rng, 64)
    pts = np.concatenate([pts, [[np.nan, 0.0], [0.0, np.inf]]]).astype(F)
    rays = np.concatenate([rays, [[0, 50, 0, 0, 100], [0, 50, 1, 0, -1], [0, 50, np.nan, 1, 100], [0, 50, 1, 0, np.inf]]]).astype(F)
    dp, dr = DeviceBuffer(pts.nbytes), DeviceBuffer(rays.nbytes)
    dp.from_host(pts); dr.from_host(rays)
    db, dh = DeviceBuffer(4 * len(pts)), DeviceBuffer(24 * len(rays))
    for skip in (False, True):
        w.query_points_device(dp.address(), len(pts), db.address(), skip_static=skip)
        w.raycast_device(dr.address(), len(rays), dh.address(), skip_static=skip)
        w.sync()
        body = db.to_host().view(np.int32)
        hit = dh.to_host().view(ray_hit_dtype)
        bodies = w.bodies
        assert body.tobytes() == spec.query_points(bodies, pts, skip).tobytes()
        assert hit.tobytes() == spec.raycast(bodies, rays, skip).tobytes()
        assert body[-2:].tolist() == [-1, -1] and hit["body"][-4:].tolist() == [-1] * 4
        assert body[:-2].tobytes() == w.query_points(pts[:-2], skip_static=skip).tobytes()
        assert hit[:-4].tobytes() == w.raycast(rays[:-4], skip_static=skip).tobytes()
    w.query_points_device(dp.address(), 0, db.address())
    assert w.L.phx_world_query_points_device(w.h, None, 1, 0, None) == -1
    assert w.L.phx_world_raycast_device(w.h, dr.address(), 1, 2, dh.address()) == -1      # (flags)


def test_pick_example_runs(tmp_path, built_lib):
    exe = str(tmp_path / "pick")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pick.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    r = subprocess.run([exe, "240"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "picked body" in r.stdout


def _segments_equal(off, hits, so, sh, sel, what):
    for j, q in enumerate(sel):
        got = hits[off[q]:off[q + 1]]
        want = sh[so[j]:so[j + 1]]
        assert got.tobytes() == want.tobytes(), "%s: box %d" % (what, q)


@pytest.mark.parametrize("chunk", ("64", "128"))
def test_scan_aabb_in_chunks(built_lib, monkeypatch, chunk):
    """The scan path's AABB table in several chunks of queries (PHX_QUERY_SCAN_CHUNK lowers the chunk on a small world): the same bytes
    as the spec, with and without SKIP_STATIC, and a count that is not a multiple of the chunk."""
    monkeypatch.setenv("PHX_QUERY_PATH", "scan")
    monkeypatch.setenv("PHX_QUERY_SCAN_CHUNK", chunk)
    w = _world(scenes.piles(3, 50, ymax=220.0))
    for _ in range(3):
        w.Update(DT, CFG)
    bodies = w.bodies
    boxes, _, _ = _queries(bodies, np.random.default_rng(int(chunk)), 150)
    assert len(boxes) > 2 * int(chunk) and len(boxes) % int(chunk)
    for skip in (False, True):
        off, hits = w.query_aabb(boxes, skip_static=skip)
        so, sh = spec.query_aabb(bodies, boxes, skip)
        assert off.tobytes() == so.tobytes() and hits.tobytes() == sh.tobytes(), "chunk %s skip=%s" % (chunk, skip)


def test_scan_aabb_beyond_one_chunk_at_cfg2(built_lib, monkeypatch):
    """90 000 boxes on the scan path at cfg 2: more than one chunk of the (query, body block) table by default (85 760 queries at 782
    body blocks).  Equal to the index path's answer, and a sample of the boxes to the spec."""
    rng = np.random.default_rng(17)
    k = 90000
    o = rng.uniform([-3000, 0], [3000, 2000], (k, 2))
    boxes = np.concatenate([o, o + rng.uniform(0, 40, (k, 2))], axis=1).astype(F)
    got = {}
    for p in ("scan", "index"):
        monkeypatch.setenv("PHX_QUERY_PATH", p)
        w = _cfg2(5)
        got[p] = w.query_aabb(boxes)
        if p == "scan":
            bodies = w.bodies
        del w
    assert got["scan"][0].tobytes() == got["index"][0].tobytes() and got["scan"][1].tobytes() == got["index"][1].tobytes()
    assert got["scan"][0][-1] > 0
    sel = np.concatenate([rng.choice(k, 100, replace=False), [0, 85759, 85760, k - 1]])
    so, sh = spec.query_aabb(bodies, boxes[sel])
    _segments_equal(got["scan"][0], got["scan"][1], so, sh, sel, "cfg 2 scan")


@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
def test_listing_protocol(built_lib, path):
    """phx_world_query_aabb with hit_cap one short and exact, and boxes that count no hit at all, on both paths."""
    w = listing_cases.world()
    bodies = w.bodies
    boxes = np.array([[-1e4, -1e4, 1e4, 1e4], [5000, 5000, 5010, 5010], [-5, 12, 5, 28]], dtype=F)      # everything, nothing, two boxes
    so, sh = spec.query_aabb(bodies, boxes)
    assert np.diff(so).tolist() == [len(bodies), 0, 2]
    listing_cases.one_short(w, "phx_world_query_aabb", "hits", boxes, so, sh)
    listing_cases.counted_none(w, "phx_world_query_aabb", np.tile(boxes[1], (3, 1)))


def test_scan_aabb_in_chunks_one_short(built_lib, monkeypatch):
    """hit_cap one short on the chunked scan: the later chunks are counted again between the offsets and the fill."""
    monkeypatch.setenv("PHX_QUERY_PATH", "scan")
    monkeypatch.setenv("PHX_QUERY_SCAN_CHUNK", "64")
    w = listing_cases.world()
    bodies = w.bodies
    boxes, _, _ = _queries(bodies, np.random.default_rng(64), 150)
    assert len(boxes) > 2 * 64 and len(boxes) % 64
    so, sh = spec.query_aabb(bodies, boxes)
    assert so[64] < so[128] < so[-1]                                    # (every chunk has hits)
    listing_cases.one_short(w, "phx_world_query_aabb", "hits", boxes, so, sh)


@pytest.mark.parametrize("var,value", [("PHX_QUERY_PATH", "indx"), ("PHX_QUERY_SCAN_CHUNK", "100"), ("PHX_QUERY_SCAN_CHUNK", "x")])
def test_unknown_knob_values_are_refused(built_lib, monkeypatch, var, value):
    monkeypatch.setenv(var, value)
    with pytest.raises(phyx_amd.PhxError, match=var):
        phyx_amd.World(0)


# ---- the directed corpus: the spec's bytes, and the judge's bounds on the device's own answers --------------------------------------------
@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
@pytest.mark.parametrize("name", [c.name for c in qc.cases() if (c.kinds == qc.BOX).any()])
def test_corpus_boxes_equal_the_spec_and_meet_the_judge(built_lib, name, path):
    """A world of the corpus case's boxes alone (no shape column, no step): raycast and query_points are byte-equal to query_spec, and
    the device's own answers meet the float64 judge by the bounds and the excused set of
    test_queries_cpu.test_spec_box_rules_against_the_float64_judge."""
    c = qc.case(name)
    w = qc.world(*qc.boxes_only(c))
    bodies = w.bodies
    kinds = np.zeros(len(bodies), dtype=np.int32)
    for rays in (c.rays, c.near_rays):
        if not len(rays):
            continue
        got, want = w.raycast(rays), spec.raycast(bodies, rays)
        assert got.tobytes() == want.tobytes(), "%s %s: rays %s" % (name, path, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[:8])
        _, worst = qc.judged("rays", qc.judge_hits, bodies, kinds, rays, got)
        if rays is c.rays:
            print("%s %s: worst in u: %s" % (name, path, qc.table(worst)))
            qc.assert_bounds(worst, "%s %s" % (name, path))
    for pts in (c.points, c.near_points):
        if not len(pts):
            continue
        got = w.query_points(pts)
        assert got.tobytes() == spec.query_points(bodies, pts).tobytes(), "%s %s: points" % (name, path)
        qc.judged("points", qc.judge_points, bodies, kinds, pts, got)


@pytest.mark.parametrize("path", ("scan", "index"), indirect=True)
@pytest.mark.parametrize("shift", ((3000.0, -7000.0), (1e5, 1e5)), ids=lambda s: "%g,%g" % s)
def test_shifted_oriented_boxes_and_casts_equal_the_spec(built_lib, shift, path):
    """The 0 .. 100 field of test_shape_queries_cpu's float64 checks, moved out to where the project's worlds reach: 64 bodies, 128
    oriented boxes and 128 casts in and around it, byte-equal to shape_query_spec."""
    rng = np.random.default_rng(20242)
    field = lambda n, lo, hi, big: np.stack([rng.uniform(lo, hi, n) + shift[0], rng.uniform(lo, hi, n) + shift[1], rng.uniform(0, 2 * np.pi, n),      # noqa: E731
                                             rng.uniform(0.5, big, n), rng.uniform(0.5, big, n)], axis=1).astype(F)
    w = phyx_amd.World(0, gravity=0.0)
    w.add_bodies(field(64, 0, 100, 20))
    bodies = w.bodies
    boxes = np.stack([phyx_amd.box_from_angle(*q) for q in field(128, -60, 160, 6)]).astype(F)      # (smaller, and around the field too: some miss)
    ang = rng.uniform(0, 2 * np.pi, 128)
    d = np.stack([np.cos(ang), np.sin(ang)], axis=1) * rng.uniform(0.5, 3.0, (128, 1))
    casts = np.concatenate([boxes, d, rng.uniform(5.0, 60.0, (128, 1))], axis=1).astype(F)
    off, hits = w.query_boxes(boxes)
    so, sh = shape_query_spec.query_boxes(bodies, boxes)
    assert off.tobytes() == so.tobytes() and hits.tobytes() == sh.tobytes(), path
    assert 0 < len(hits) < 64 * 128
    got = w.cast_boxes(casts)
    assert got.tobytes() == shape_query_spec.cast_boxes(bodies, casts).tobytes(), path
    assert 0 < (got["body"] >= 0).sum() < 128
