"""The nearest-body query without a GPU (include/phyx_amd.h, QUERIES: phx_world_query_nearest): tests/near_spec.py, the definition,
held to the float64 judge on the directed corpus (tests/near_corpus.py) with its bounds and its cap; the pruning argument of the
header as tests (D >= la bit for bit, node bounds below their bodies', a walk that skips by the running bound returns the scan's
bytes in any order); the rule's conventions on small exact cases; the Python wrapper's refusals and the ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import near_corpus as nc
import near_spec as spec
import polygon_spec as ps
import reach_example
from phyx_amd.api import near_hit_dtype
from query_corpus import records
from query_spec import Geometry

F = np.float32
FLT_MAX = nc.FLT_MAX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("phx_world_query_nearest", "phx_world_query_nearest_device")
BOX, CIRCLE, CAPSULE, POLYGON = 0, 1, 2, 3


# ---- the specification against the judge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in nc.cases()])
def test_spec_against_the_float64_judge(name):
    """Every clear query names the judge's body; every measure of every named body is within its bound; the excused share of the
    (query, body) pairs stays under the cap.  The doubtful queries are excused or right."""
    c = nc.case(name)
    got = spec.query_nearest(c.bodies, c.kinds, c.polys, c.queries)
    pairs, worst = nc.judge_near(c.bodies, c.kinds, c.polys, c.queries, got)
    print("%s: %d queries, excused %.4f, worst in u: %s" % (name, len(c.queries), pairs.mean(), nc.table(worst)))
    assert pairs.mean() <= nc.CAP
    nc.assert_bounds(worst, name)
    assert (got["body"] >= 0).sum() >= 20                                    # (the -1s: max_dist DESIGN u short of the distance)
    if len(c.near_queries):
        near = spec.query_nearest(c.bodies, c.kinds, c.polys, c.near_queries)
        nc.assert_bounds(nc.judge_near(c.bodies, c.kinds, c.polys, c.near_queries, near)[1], name + " (doubtful)")


def test_the_corpus_reaches_every_kind_region_and_verdict():
    c = nc.case("near the origin")
    B = c.B
    got = spec.query_nearest(c.bodies, c.kinds, c.polys, c.queries)
    seen = set()
    for q, row in enumerate(c.queries):
        v = nc.ref.near(B, row)
        b = int(got["body"][q])
        seen.add((int(B.kind[b]), v.region[b], bool(v.sd[b] < 0)))
    want = {(BOX, "face", False), (BOX, "corner", False), (BOX, "face", True), (CIRCLE, "round", False), (CIRCLE, "round", True),
            (CAPSULE, "round", False), (CAPSULE, "round", True), (POLYGON, "face", False), (POLYGON, "corner", False), (POLYGON, "face", True)}
    assert seen >= want, want - seen
    assert (c.queries[:, 2] == F(FLT_MAX)).sum() > 100
    near = spec.query_nearest(c.bodies, c.kinds, c.polys, c.near_queries)
    assert (near["body"] == -1).any() and (near["body"] >= 0).any()         # (max_dist one ulp short of the distance, and at it)
    row = nc.case("a row, the nearer has the higher index")
    verdicts = []
    got = spec.query_nearest(row.bodies, row.kinds, row.polys, row.queries, verdicts=verdicts)
    beaten = [q for q, (D, cand) in enumerate(verdicts) if cand[0] and got["body"][q] > 0]
    assert len(beaten) >= 8 and len(set(got["body"].tolist())) == 6         # body 0 was a candidate and a higher index was nearer


# ---- the pruning argument ---------------------------------------------------------------------------------------------------------------
def random_world(seed, n=192, at=0.0):
    """n bodies of the four kinds around (at, at): angles that include the exact frames, sizes 0.3 .. 12."""
    rng = np.random.default_rng(seed)
    gons = nc.polygons()
    rows, polys = [], []
    for i in range(n):
        kind = int(rng.integers(0, 4))
        ang = ("0", "pi/2", float(rng.uniform(0, 6.3)), float(rng.uniform(-1e-3, 1e-3)))[int(rng.integers(0, 4))]
        hx, hy = (float(v) for v in rng.uniform(0.3, 12.0, 2))
        poly = None
        if kind == CIRCLE:
            hy = hx
        elif kind == CAPSULE:
            hx, hy = max(hx, hy) + 0.1, min(hx, hy)
        elif kind == POLYGON:
            poly = gons[int(rng.integers(0, 4))]
            hx, hy = (float(v) for v in ps.frame_box(poly))
        rows.append((at + float(rng.uniform(-150, 150)), at + float(rng.uniform(-150, 150)), ang, hx, hy, kind))
        polys.append(poly)
    bodies, kinds = records(rows)
    return bodies, kinds, polys


def random_points(seed, k, at=0.0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(at - 250, at + 250, (k, 2))
    return np.concatenate([p, rng.choice([0.0, 2.0, 50.0, FLT_MAX], (k, 1))], axis=1).astype(F)


@pytest.mark.parametrize("at", (0.0, 1e5))
def test_the_reported_distance_is_never_below_the_aabb_gap(at):
    """D_b >= la_b bit for bit wherever la_b > 0, on all four kinds, exact frames and bodies at 10^5 included; and sd alone would
    not do: in float32 it does fall short of la."""
    short = total = 0
    for seed in range(3):
        bodies, kinds, polys = random_world(seed, at=at)
        g = Geometry(bodies)
        for x, y, _ in random_points(100 + seed, 150, at):
            sd = spec.shape(g, kinds, polys, x, y)[0]
            la = spec.gap(g, x, y)
            D = spec.distance(sd, la)
            out = la > 0
            assert (D[out] >= la[out]).all()
            assert (D[~out] == np.where(sd[~out] == 0, F(0), sd[~out])).all()
            assert not np.signbit(D[D == 0]).any()
            short += int((sd[out] < la[out]).sum())
            total += int(out.sum())
    assert total > 50000 and short > 0, (short, total)


def test_node_bounds_never_exceed_their_bodies():
    """The numpy model of the tree's bounds (unions of 64 AABBs, two levels): la_node <= la_b for every body below the node, so a node
    skipped by la_node > best D holds no body with D <= best D."""
    bodies, kinds, polys = random_world(7, n=64 * 5 + 17)
    g = Geometry(bodies)
    order = np.random.default_rng(7).permutation(g.n)
    l1, l2 = spec.node_bounds(g, order)
    assert len(l1[0]) == 6 and len(l2[0]) == 1
    for x, y, _ in random_points(8, 200):
        la = spec.gap(g, x, y)[order]
        la1 = spec.box_gap(*l1, x, y)
        la2 = spec.box_gap(*l2, x, y)
        assert (np.repeat(la1, 64)[:g.n] <= la).all() and (la2[0] <= la1).all()


@pytest.mark.parametrize("at", (0.0, 1e5))
def test_a_walk_that_skips_by_the_running_bound_returns_the_scans_bytes(at):
    """Several shuffled visiting orders over two shuffled body orders, every max_dist of the device tests: the bytes of the plain
    statement of the rule, ties included (the world holds every body twice), and the bound does skip leaves."""
    bodies, kinds, polys = random_world(11, n=160, at=at)
    bodies, kinds, polys = np.concatenate([bodies, bodies]), np.concatenate([kinds, kinds]), polys + polys      # (exact ties between b and b + 160)
    queries = random_points(12, 60, at)
    want = spec.query_nearest(bodies, kinds, polys, queries)
    assert (want["body"] >= 0).sum() > 20 and (want["body"] < 160).all()
    leaves = 0
    for seed in range(3):
        rng = np.random.default_rng(seed)
        visited = []
        got = spec.walk(bodies, kinds, polys, queries, rng.permutation(len(bodies)), rng, visited=visited)
        assert got.tobytes() == want.tobytes(), "order %d" % seed
        leaves += sum(visited)
    assert leaves < 3 * 60 * 5


# ---- the rule's conventions, on cases small enough to know the answer ---------------------------------------------------------------------
def _one(row, poly=None):
    b, k = records([row])
    return b, k, [poly]


def test_spec_exact_answers_on_an_aligned_box():
    b, k, p = _one((10.0, 20.0, "0", 4.0, 3.0, BOX))
    q = [[17.0, 20.0, 10.0], [10.0, 26.0, 10.0], [17.0, 27.0, 10.0], [11.0, 20.5, 10.0], [10.0, 20.0, 10.0], [3.0, 20.0, 2.0], [13.0, 22.0, 0.0]]
    out = spec.query_nearest(b, k, p, q)
    assert out["body"].tolist() == [0, 0, 0, 0, 0, -1, 0]
    assert out["distance"].tolist() == [3.0, 3.0, 5.0, -2.5, -3.0, 0.0, -1.0]
    assert out["normal"].tolist() == [[1, 0], [0, 1], [F(3.0) / F(5.0), F(4.0) / F(5.0)], [0, 1], [0, 1], [0, 0], [1, 0]]
    assert out["point"].tolist() == [[14, 20], [10, 23], [14, 23], [11, 23], [10, 23], [0, 0], [14, 22]]
    assert out[5].tobytes() == spec.query_nearest(b[:0], None, [], q[5:6])[0].tobytes()      # none: body -1, every other field 0


def test_spec_circle_capsule_and_polygon():
    b, k, p = _one((0.0, 0.0, "0", 2.0, 2.0, CIRCLE))
    out = spec.query_nearest(b, k, p, [[5.0, 0.0, 10.0], [0.0, -1.0, 10.0], [0.0, 0.0, 10.0]])
    assert out["distance"].tolist() == [3.0, -1.0, -2.0] and out["normal"].tolist() == [[1, 0], [0, -1], [0, 0]]
    assert out["point"].tolist() == [[2, 0], [0, -2], [0, 0]]              # the centre: normal (0, 0), point pos
    b, k, p = _one((0.0, 0.0, "0", 3.0, 1.0, CAPSULE))
    out = spec.query_nearest(b, k, p, [[1.0, 4.0, 10.0], [6.0, 0.0, 10.0], [1.5, 0.0, 10.0], [2.0, 0.5, 10.0]])
    assert out["distance"].tolist() == [3.0, 3.0, -1.0, -0.5] and out["normal"].tolist() == [[0, 1], [1, 0], [0, 0], [0, 1]]
    assert out["point"].tolist() == [[1, 1], [3, 0], [1.5, 0], [2, 1]]     # on the core: normal (0, 0) and the core's point
    b, k, p = _one((0.0, 0.0, "0", 10.0, 0.5, POLYGON), nc.polygons()[3])
    out = spec.query_nearest(b, k, p, [[0.0, 2.5, 10.0], [13.0, 4.5, 10.0], [2.0, 0.25, 10.0]])
    assert out["distance"].tolist() == [2.0, 5.0, -0.25] and out["point"].tolist() == [[0, 0.5], [10, 0.5], [2, 0.5]]
    assert out["normal"][1].tolist() == [F(3.0) / F(5.0), F(4.0) / F(5.0)] and out["normal"][2].tolist() == [0, 1]


def test_spec_ties_skip_static_nan_and_the_device_form_rules():
    b, k = records([(0.0, 0.0, "0", 1.0, 1.0, BOX), (10.0, 0.0, "0", 1.0, 1.0, CIRCLE), (10.0, 0.0, "0", 1.0, 1.0, CIRCLE)])
    p = [None] * 3
    out = spec.query_nearest(b, k, p, [[5.0, 0.0, 100.0], [9.0, 5.0, FLT_MAX]])
    assert out["body"].tolist() == [0, 1] and out["distance"][0] == 4.0    # equal D: the lowest index; identical bodies: the lowest index
    b["inv_mass"][0] = b["inv_inertia"][0] = 0
    assert spec.query_nearest(b, k, p, [[5.0, 0.0, 100.0]], skip_static=True)["body"].tolist() == [1]
    b["aabb_min"]["x"][1] = np.nan
    assert spec.query_nearest(b, k, p, [[9.0, 5.0, FLT_MAX]])["body"].tolist() == [2]      # a NaN AABB is no candidate
    bad = [[np.nan, 0, 1], [0, np.inf, 1], [0, 0, -1.0], [0, 0, np.inf], [0, 0, np.nan]]
    assert spec.query_nearest(b, k, p, bad).tobytes() == spec.query_nearest(b[:0], None, [], bad).tobytes()
    assert spec.query_nearest(b, k, p, [[0.5, 0.0, 0.0]])["body"].tolist() == [0]          # max_dist == 0 finds what holds the point
    far = spec.query_nearest(b, k, p, [[1e18, -1e18, FLT_MAX], [-3e5, 4e5, FLT_MAX], [3e30, 0.0, FLT_MAX]])
    assert far["body"][0] >= 0 and far["body"].tolist()[1:] == [0, -1] and far["distance"][0] > 1e18      # FLT_MAX: anywhere, max_dist overflows nothing ...
    assert np.isfinite(far["distance"]).all()                                             # ... (a point whose own squares overflow is at +inf: none)


def test_distance_is_never_minus_zero():
    b, k, p = _one((0.0, 0.0, "0", 10.0, 0.5, POLYGON), nc.polygons()[3])
    out = spec.query_nearest(b, k, p, [[10.0, 0.0, 1.0], [0.0, -0.5, 1.0]])               # on the surface: the edges' normals hold -0
    assert out["distance"].tolist() == [0.0, 0.0] and not np.signbit(out["distance"]).any()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
class _NoC:
    """Stands in for the library: any call into C fails the test."""

    def __getattr__(self, name):
        raise AssertionError("%s was called with input the wrapper should have refused" % name)


def _world(lib=None):
    from phyx_amd import World
    w = World.__new__(World)
    w.L, w.h = lib if lib is not None else _NoC(), None
    return w


BAD = {"shape": np.zeros((3, 2), dtype=F), "one row": np.zeros(3, dtype=F), "nan": [[np.nan, 0, 1]], "inf": [[0, np.inf, 1]],
       "beyond float": [[1e39, 0, 1]], "max_dist < 0": [[0, 0, -2]], "nan max_dist": [[0, 0, np.nan]], "inf max_dist": [[0, 0, np.inf]],
       "bool": np.zeros((1, 3), dtype=bool), "text": [["a"] * 3]}


@pytest.mark.parametrize("rule", sorted(BAD))
def test_query_nearest_refuses_bad_input(rule):
    with pytest.raises((TypeError, ValueError)):
        _world().query_nearest(BAD[rule])


class _Recorder:
    def __init__(self):
        self.calls = []

    def phx_world_query_nearest(self, h, queries, count, flags, out):
        self.calls.append((count, flags))
        return 0


def test_query_nearest_passes_good_input_on():
    rec = _Recorder()
    out = _world(rec).query_nearest([[0, 0, 0], [1, 2, FLT_MAX]], skip_static=True)
    assert rec.calls == [(2, 1)] and out.dtype == near_hit_dtype and len(out) == 2
    assert len(_world(rec).query_nearest([])) == 0


def test_near_hit_dtype_is_the_headers_record():
    assert near_hit_dtype.itemsize == 24 and near_hit_dtype.names == ("body", "distance", "normal", "point")
    import phyx_amd
    assert phyx_amd.near_hit_dtype is near_hit_dtype


def test_null_handle_is_an_error(built_lib):
    L = built_lib
    q = np.zeros(3, dtype=F)
    out = np.zeros(1, dtype=near_hit_dtype)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.phx_world_query_nearest(None, vp(q), 1, 0, vp(out)) == -1
    assert L.phx_world_query_nearest_device(None, vp(q), 1, 0, vp(out)) == -1
    assert b"null handle" in L.phx_last_error()


def test_reach_example_compiles_and_fails_loudly_without_a_gpu(tmp_path, built_lib):
    import phyx_amd
    exe = reach_example.build(tmp_path)
    try:
        have_gpu = phyx_amd.device_count() > 0
    except phyx_amd.PhxError:
        have_gpu = False
    if have_gpu:
        return                                                          # (its run is the gpu test's)
    r = subprocess.run([exe, "10"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "no CPU fallback" in r.stderr


def test_header_binding_and_library_agree_on_the_two_symbols(built_lib):
    from phyx_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "phyx_amd.h")).read()
    assert re.search(r"typedef struct \{ int32_t body; float distance; phx_vec2 normal, point; \} phx_near_hit;", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "phyx_amd", "libphyx_amd.so")], text=True)
    for name in SYMBOLS:
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert decl, "%s is not declared in include/phyx_amd.h" % name
        assert name in _lib.declared_symbols() and hasattr(built_lib, name)
        assert re.search(r"\bT %s$" % name, out, flags=re.M), "%s is not exported" % name
        fn = getattr(built_lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(decl.group(1).split(",")), name
    assert built_lib.phx_abi_version() == 2
