"""Shape queries on the device (include/phyx_amd.h, QUERIES: phx_world_query_boxes / phx_world_cast_boxes) held byte for byte to
tests/shape_query_spec.py on both paths: the edges of the tree's levels with a query mix that reaches every kind of result, the scan
path's chunks, a stepped pile queried with its own records, the capacity rule, the device form, answers after every kind of change,
no effect on the world, the host forms' refusals and examples/place.c."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import listing_cases
import phyx_amd
import shape_query_spec as spec
from phyx_amd import Configuration, DeviceBuffer, scenes
from phyx_amd.api import box_from_angle, shape_hit_dtype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _columns(b):
    pos = np.stack([b["pos"]["x"], b["pos"]["y"]], axis=1).astype(F)
    xv = np.stack([b["xv"]["x"], b["xv"]["y"]], axis=1).astype(F)
    yv = np.stack([b["yv"]["x"], b["yv"]["y"]], axis=1).astype(F)
    h = np.stack([b["geom_size"]["x"], b["geom_size"]["y"]], axis=1).astype(F)
    return pos, xv, yv, h


def _own_boxes(b):
    """The bodies' own boxes as query boxes: exact copies of the stored floats."""
    return np.concatenate(_columns(b), axis=1).astype(F)


def _random(bodies, rng, k):
    """k seeded boxes and k casts over the extent of the bodies that can move (a ground is 20 000 wide), of all of them when none can,
    and over a 100-unit square when there are none."""
    moving = bodies[(bodies["inv_mass"] != 0) | (bodies["inv_inertia"] != 0)]
    bodies = moving if len(moving) else bodies
    n = len(bodies)
    lo = np.array([bodies["aabb_min"]["x"].min(), bodies["aabb_min"]["y"].min()], dtype=np.float64) if n else np.zeros(2)
    hi = np.array([bodies["aabb_max"]["x"].max(), bodies["aabb_max"]["y"].max()], dtype=np.float64) if n else np.full(2, 100.0)
    c = rng.uniform(lo - 10.0, hi + 10.0, size=(k, 2))
    boxes = np.stack([box_from_angle(x, y, a, hx, hy) for (x, y), a, hx, hy in
                      zip(c, rng.uniform(0, 2 * np.pi, k), rng.uniform(0.5, 12.0, k), rng.uniform(0.5, 12.0, k))])
    ang = rng.uniform(0, 2 * np.pi, k)
    speed = rng.uniform(0.5, 3.0, k)
    casts = np.concatenate([boxes[rng.permutation(k)], (np.cos(ang) * speed)[:, None], (np.sin(ang) * speed)[:, None], rng.uniform(0.0, 120.0, (k, 1))], axis=1)
    return boxes.astype(F), casts.astype(F)


def _directed(bodies, b):
    """Casts aimed at body b that reach each kind of result when nothing else is in the way: a start inside, entry through the body's
    two axes (a small box meets a face of the body) and through the query's two axes (a corner of the body meets a face of a large,
    turned query box), and a cast that stops short."""
    pos, xv, yv, h = (c[b].astype(np.float64) for c in _columns(bodies))
    small = lambda p: box_from_angle(p[0], p[1], 0.6, 0.1, 0.1)           # noqa: E731
    out = [np.concatenate([small(pos), [1.0, 0.5, 10.0]]),                                          # inside
           np.concatenate([small(pos - 30.0 * xv), xv, [100.0]]),                                   # the face whose normal is xv
           np.concatenate([small(pos - 30.0 * yv), yv, [100.0]]),                                   # ... yv
           np.concatenate([small(pos - 30.0 * xv), xv, [5.0]])]                                     # stops short
    for angle, axis in ((0.6, 0), (-0.6, 1)):
        q = box_from_angle(0.0, 0.0, angle, 10.0, 10.0).astype(np.float64)
        d = q[2:4] if axis == 0 else q[4:6]                             # along the query's own X / Y: both point up and to the right
        q[0:2] = pos - 40.0 * d
        out.append(np.concatenate([q, d, [100.0]]))
    return np.stack(out).astype(F)


def _check(w, boxes, casts, what="", skips=(False, True)):
    bodies = w.bodies
    for skip in skips:
        off, hits = w.query_boxes(boxes, skip_static=skip)
        so, sh = spec.query_boxes(bodies, boxes, skip)
        assert off.tobytes() == so.tobytes() and hits.tobytes() == sh.tobytes(), "query_boxes %s skip=%s" % (what, skip)
        got, want = w.cast_boxes(casts, skip_static=skip), spec.cast_boxes(bodies, casts, skip)
        assert got.tobytes() == want.tobytes(), "cast_boxes %s skip=%s: first differing cast %s" % (
            what, skip, next((i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()), None))
    return bodies


def _grid(n):
    """n rotated boxes on a grid (as test_queries_gpu.test_level_edges): body 0 is the lower left corner."""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    return np.stack([(k % side) * 9.0, (k // side) * 9.0 + 20.0, k * 0.01, np.full(n, 4.0), np.full(n, 3.0)], axis=1).astype(F)


@pytest.mark.parametrize("n", (0, 1, 64, 65, 4096, 4097))
def test_level_edges(built_lib, path, n):
    """40 random boxes and 40 random casts (and, with bodies, the directed casts at body 0, which nothing hides from below and from the
    left) on worlds at the edges of the tree's levels.  The spec's own answers show every kind of result: no hit, a hit from inside and
    entry through each of the four axes (an empty world can only give the first)."""
    w = phyx_amd.World(0, gravity=G)
    if n:
        w.add_bodies(_grid(n))
    w.Update(DT, CFG)
    rng = np.random.default_rng(n)
    boxes, casts = _random(w.bodies, rng, 40)
    if n:
        casts = np.concatenate([casts, _directed(w.bodies, 0)])
    bodies = _check(w, boxes, casts, what="n=%d" % n)
    kinds = []
    spec.cast_boxes(bodies, casts, detail=kinds)
    assert set(kinds) == ({None, -1, 0, 1, 2, 3} if n else {None}), kinds
    off, hits = spec.query_boxes(bodies, boxes)
    assert (off[-1] > 0) == (n > 0)
    off, hits = w.query_boxes(np.zeros((0, 8), dtype=F))
    assert off.tolist() == [0] and len(hits) == 0 and len(w.cast_boxes(np.zeros((0, 11), dtype=F))) == 0


def _stepped(scene, steps):
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scene)
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
        w = _stepped(scenes.falling(299, width=80.0, ymax=260.0), 3)
        assert w.counts()[0] == 300
        boxes, _ = _random(w.bodies, np.random.default_rng(count), count)
        got[chunk] = [w.query_boxes(boxes, skip_static=skip) for skip in (False, True)]
        if chunk:
            for skip in (False, True):
                so, sh = spec.query_boxes(w.bodies, boxes, skip)
                assert got[chunk][skip][0].tobytes() == so.tobytes() and got[chunk][skip][1].tobytes() == sh.tobytes()
    for a, b in zip(got[None], got["64"]):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0][-1] > 0


def test_stepped_scene(built_lib, path):
    """A pile of rotated boxes after 30 steps (arbitrary frames): random queries, and queries built from the bodies' own records: a
    body's own box (it hits itself and what it rests on), the same box moved by exactly its width (an exact touch in real arithmetic),
    casts of a body's own box (t = 0) and of its copy from above."""
    w = _stepped(scenes.tilted(300), 30)
    bodies = w.bodies
    rng = np.random.default_rng(30)
    boxes, casts = _random(bodies, rng, 150)
    pick = rng.integers(0, len(bodies), 60)
    own = _own_boxes(bodies[pick])
    pos, xv, yv, h = _columns(bodies[pick])
    beside = own.copy()
    beside[:, 0:2] = pos + xv * (h[:, :1] + h[:, :1])
    above = own.copy()
    above[:, 0:2] = pos + yv * F(40.0)
    boxes = np.concatenate([boxes, own, beside])
    casts = np.concatenate([casts,
                            np.concatenate([own, np.tile([0.0, -1.0, 50.0], (60, 1))], axis=1),
                            np.concatenate([above, -yv, np.full((60, 1), 100.0)], axis=1),
                            np.concatenate([beside, -xv, np.full((60, 1), 1.0)], axis=1)]).astype(F)
    _check(w, boxes.astype(F), casts, what="tilted after 30 steps")
    off, _ = spec.query_boxes(bodies, own)
    assert (np.diff(off) >= 1).all()                                    # every body overlaps at least itself
    assert (spec.cast_boxes(bodies, casts[150:210])["t"] == 0).all()


def test_capacity(built_lib, path):
    w = _stepped(scenes.wall(14, 12), 3)
    bodies = w.bodies
    boxes, _ = _random(bodies, np.random.default_rng(8), 30)
    so, sh = spec.query_boxes(bodies, boxes)
    total = int(so[-1])
    assert total > 2
    offsets, out, t = np.zeros(31, dtype=np.int32), np.zeros(total, dtype=np.int32), C.c_int64(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert w.L.phx_world_query_boxes(w.h, vp(boxes), 30, 0, vp(offsets), vp(out), total - 1, C.byref(t)) == -4
    assert t.value == total and offsets.tobytes() == so.tobytes()
    assert w.L.phx_world_query_boxes(w.h, vp(boxes), 30, 0, vp(offsets), vp(out), int(t.value), C.byref(t)) == 0
    assert out.tobytes() == sh.tobytes() and offsets.tobytes() == so.tobytes()
    n = len(bodies)
    off, hits = w.query_boxes(np.tile(box_from_angle(0.0, 50.0, 0.3, 500.0, 500.0), (8, 1)))      # (the wrapper's retry: 8 n > 1024 hits)
    assert 8 * n > 1024 and off.tolist() == [n * k for k in range(9)] and hits.tolist() == list(range(n)) * 8


def test_listing_protocol(built_lib, path):
    """phx_world_query_boxes with hit_cap one short and exact, and boxes that count no hit at all, on both paths."""
    w = listing_cases.world()
    bodies = w.bodies
    boxes = np.stack([box_from_angle(0.0, 100.0, 0.3, 500.0, 500.0), box_from_angle(5000.0, 5000.0, 0.3, 2.0, 2.0),
                      box_from_angle(0.0, 20.0, 0.3, 4.0, 4.0)]).astype(F)                            # everything, nothing, two boxes
    so, sh = spec.query_boxes(bodies, boxes)
    assert np.diff(so).tolist() == [len(bodies), 0, 2]
    listing_cases.one_short(w, "phx_world_query_boxes", "hits", boxes, so, sh)
    listing_cases.counted_none(w, "phx_world_query_boxes", np.tile(boxes[1], (3, 1)))


def test_device_form(built_lib, path):
    w = _stepped(scenes.wall(14, 12), 3)
    _, casts = _random(w.bodies, np.random.default_rng(4), 64)
    ok = casts[0].copy()
    bad = np.tile(ok, (7, 1))
    bad[0, 8:10] = 0.0                                                 # d == (0, 0)
    bad[1, 10] = -1.0                                                  # max_t < 0
    bad[2, 3] = np.nan
    bad[3, 10] = np.inf
    bad[4, 6] = 0.0                                                    # h.x == 0
    bad[5, 7] = -2.0
    bad[6, 0] = -np.inf
    casts = np.concatenate([casts, bad]).astype(F)
    dc, dh = DeviceBuffer(casts.nbytes), DeviceBuffer(16 * len(casts))
    dc.from_host(casts)
    for skip in (False, True):
        w.cast_boxes_device(dc.address(), len(casts), dh.address(), skip_static=skip)
        w.sync()
        hit = dh.to_host().view(shape_hit_dtype)
        assert hit.tobytes() == spec.cast_boxes(w.bodies, casts, skip).tobytes()
        assert hit[:-7].tobytes() == w.cast_boxes(casts[:-7], skip_static=skip).tobytes()
        assert hit[-7:].tobytes() == spec.cast_boxes(w.bodies[:0], bad).tobytes()      # body -1, every other field 0
    assert (hit["body"][:-7] >= 0).any()
    w.cast_boxes_device(dc.address(), 0, dh.address())
    assert w.L.phx_world_cast_boxes_device(w.h, None, 1, 0, None) == -1
    assert w.L.phx_world_cast_boxes_device(w.h, dc.address(), 1, 2, dh.address()) == -1      # (flags)


def test_staleness(built_lib, path):
    """Query, change, query again: every answer is the spec of the world as it is then."""
    rng = np.random.default_rng(5)
    w = phyx_amd.World(0, gravity=G)
    w.add_scene(scenes.piles(3, 50, ymax=220.0))

    def check(what):
        boxes, casts = _random(w.bodies, rng, 32)
        _check(w, boxes, casts, what=what, skips=(False,))

    check("host-staged, before the first step")
    w.Update(DT, CFG)
    check("after a step")
    n = w.counts()[0]
    idx = rng.choice(n, 20, replace=False)
    w.set_poses(idx, np.stack([rng.uniform(-300, 300, 20), rng.uniform(0, 400, 20), rng.uniform(0, 6, 20)], axis=1).astype(F))
    check("after set_poses")
    moved = _own_boxes(w.bodies[idx])
    off, hits = w.query_boxes(moved)
    assert all(b in hits[off[k]:off[k + 1]] for k, b in enumerate(idx))                      # the new poses are what the queries see
    w.remove_bodies(rng.choice(w.counts()[0], 25, replace=False))
    check("after remove_bodies")
    first = w.counts()[0]
    w.add_bodies(np.array([[x, 150.0, 0.3, 6.0, 4.0] for x in np.linspace(-200, 200, 30)], dtype=F))
    check("after add_bodies")
    off, hits = w.query_boxes(_own_boxes(w.bodies[first:]))
    assert all(first + k in hits[off[k]:off[k + 1]] for k in range(30))                      # the spawned bodies are there
    w.Update(DT, CFG)
    check("after another step")


def test_queries_change_nothing(built_lib, path):
    """A world answering shape queries between every step stays byte-equal to a twin that makes none, keeps its cached schedule, and
    builds the query index only when the geometry changed."""
    rng = np.random.default_rng(9)
    cfg = Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_SINGLE, 15, 15)
    a, b = phyx_amd.World(0, gravity=0.0), phyx_amd.World(0, gravity=0.0)
    a.add_scene(scenes.stack(6, 10)); b.add_scene(scenes.stack(6, 10))
    a.query_boxes([box_from_angle(0.0, 20.0, 0.1, 3.0, 3.0)])          # (before the first step: host-staged bodies go up)
    for s in range(20):
        boxes, casts = _random(b.bodies, rng, 16)                      # (from the twin: a makes nothing but the queries)
        builds = a.query_index()
        a.query_boxes(boxes); a.cast_boxes(casts, skip_static=True); a.query_boxes(boxes, skip_static=True)
        assert a.query_index() == builds, "step %d: the geometry did not change" % s
        a.Update(DT, cfg)
        b.Update(DT, cfg)
        assert a.solver.stats().recoloured == b.solver.stats().recoloured, "step %d" % s
    assert a.build_counts() == b.build_counts()
    for x, y in zip(a.state(), b.state()):
        assert x.tobytes() == y.tobytes()
    assert a.solver.stats().recoloured == 0


def test_host_forms_refuse_bad_input(built_lib):
    """PHX_ERR_INVALID before anything is queued, one rule at a time; count == 0 is valid."""
    w = _stepped(scenes.stack(2, 3), 1)
    L = w.L
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    good = np.concatenate([box_from_angle(0.0, 20.0, 0.2, 3.0, 2.0), [0.0, -1.0, 10.0]]).astype(F)
    offsets, hits, t = np.zeros(2, dtype=np.int32), np.zeros(16, dtype=np.int32), C.c_int64(0)
    out = np.zeros(1, dtype=shape_hit_dtype)
    assert L.phx_world_query_boxes(w.h, vp(good), 1, 0, vp(offsets), vp(hits), 16, C.byref(t)) == 0
    assert L.phx_world_cast_boxes(w.h, vp(good), 1, 0, vp(out)) == 0 and out["body"][0] >= 0
    for col, value in ((0, np.nan), (3, np.inf), (6, 0.0), (7, -1.0), (6, np.nan)):
        q = good.copy(); q[col] = value
        assert L.phx_world_query_boxes(w.h, vp(q), 1, 0, vp(offsets), vp(hits), 16, C.byref(t)) == -1, (col, value)
        assert L.phx_world_cast_boxes(w.h, vp(q), 1, 0, vp(out)) == -1, (col, value)
    for cols, value in (((10,), -1.0), ((10,), np.inf), ((8,), np.nan), ((8, 9), 0.0), ((8, 9), -0.0)):
        q = good.copy(); q[list(cols)] = value
        assert L.phx_world_cast_boxes(w.h, vp(q), 1, 0, vp(out)) == -1, (cols, value)
    assert L.phx_world_query_boxes(w.h, vp(good), 1, 2, vp(offsets), vp(hits), 16, C.byref(t)) == -1      # (flags)
    assert L.phx_world_query_boxes(w.h, vp(good), -1, 0, vp(offsets), vp(hits), 16, C.byref(t)) == -1
    assert L.phx_world_query_boxes(w.h, vp(good), 1, 0, None, vp(hits), 16, C.byref(t)) == -1
    assert L.phx_world_cast_boxes(w.h, vp(good), 1, 0, None) == -1
    assert L.phx_world_cast_boxes(w.h, None, 0, 0, None) == 0
    with pytest.raises(ValueError):
        w.cast_boxes([good[:8].tolist() + [0.0, 0.0, 1.0]])


def test_place_example_runs(tmp_path, built_lib):
    """The emitter that looks first: the program queries the slot again after each spawn and fails if anything but the new body is
    there; it must have spawned, and must have been refused once the pile reached the slot."""
    exe = str(tmp_path / "place")
    lib_dir = os.path.join(ROOT, "phyx_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "place.c"), "-L" + lib_dir, "-lphyx_amd", "-Wl,-rpath," + lib_dir, "-lm", "-o", exe])
    r = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spawned into an occupied slot" not in r.stderr
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("place:"))
    spawned, refused = int(line.split()[1]), int(line.split()[4])
    assert spawned >= 2 and refused >= 1 and spawned + refused == 300
    assert "touches body" in r.stdout and "touches body -1" not in r.stdout
