"""Convex polygon bodies on the CPU (include/phyx_amd.h POLYGONS): phx_debug_update_manifold_polygons — the host instantiation of the
narrowphase function the device kernel calls — against tests/polygon_spec.py byte for byte on the directed corpus
(tests/polygon_corpus.py) and on random pairs, the corpus's claims, the spec against its float64 judge (tests/polygon_reference.py),
pairs without a polygon against phx_debug_update_manifold, validity, the mass helper, and the polygon predicates of the point and ray
queries against the judge."""
import ctypes as C

import numpy as np
import pytest

import polygon_corpus as pc
import polygon_reference as ref
import polygon_spec as spec
import capsule_corpus as kc
import query_corpus as qc
from phyx_amd.api import contact_point_dtype, manifold_dtype, polygon_inverse_masses, rigid_body_dtype
from test_circles_cpu import debug_update_manifold

F = np.float32
MEASURES = ("length", "normal", "depth", "surface")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def debug_update_manifold_polygons(lib, b1, k1, p1, b2, k2, p2, count, pts):
    """(point_count, pts) after phx_debug_update_manifold_polygons."""
    r1, r2 = np.array([b1], dtype=rigid_body_dtype), np.array([b2], dtype=rigid_body_dtype)
    m = np.zeros(1, dtype=manifold_dtype)
    m["body1"], m["body2"], m["point_count"], m["point_index"] = 0, 1, count, 0
    p = np.array(pts, dtype=contact_point_dtype).copy()
    q1 = None if p1 is None else np.array([p1], dtype=spec.polygon_dtype)
    q2 = None if p2 is None else np.array([p2], dtype=spec.polygon_dtype)
    rc = lib.phx_debug_update_manifold_polygons(_ptr(r1), int(k1), None if q1 is None else _ptr(q1), _ptr(r2), int(k2), None if q2 is None else _ptr(q2),
                                                _ptr(m), _ptr(p))
    assert rc == 0, lib.phx_last_error()
    assert (m["body1"][0], m["body2"][0], m["point_index"][0]) == (0, 1, 0)
    return int(m["point_count"][0]), p


@pytest.fixture(scope="module")
def cases():
    return pc.cases()


def trace_of(c):
    t = {}
    hits = spec.contacts(spec.Body(c.b1, c.k1, c.p1), spec.Body(c.b2, c.k2, c.p2), t)
    if c.group == "capsule/polygon" and "first" not in t:
        t.update(first=None, second=None, rejected=[], sep_tie=False, depth_tie=False)
    return hits, t


def test_corpus_reaches_every_arm(cases):
    names = [c.name for c in cases]
    assert len(names) == len(set(names))
    seen = {}
    for c in cases:
        hits, t = trace_of(c)
        for key, want in c.arm.items():
            assert t.get(key) == want, "%s: %s is %r, the case claims %r (%s)" % (c.name, key, t.get(key), want, t)
        if c.group == "cache":
            continue
        order = "b2" if c.name.endswith("_b2") else "b1"
        marks = []
        if c.group == "polygon/polygon":
            marks = ["ref:%s" % t["ref"], "kept:%d" % t["kept"]] + ["clip:" + x for x in t["clips"]] + [k for k in ("ab_tie", "face_tie", "inc_tie", "touch") if t[k]]
            marks.append("sides:%d+%d" % tuple(sorted((spec.Body(c.b1, c.k1, c.p1).count, spec.Body(c.b2, c.k2, c.p2).count))))
            marks.append("box" if spec.BOX in (c.k1, c.k2) else "polygons")
        elif c.group == "circle/polygon":
            marks = ["region:%s" % t["region"]] + [k for k in ("tie", "t0", "tee", "touch") if t[k]]
        else:
            kind = lambda n: None if n is None else n.rstrip("01234567")      # noqa: E731
            marks = ["first:%s" % kind(t["first"]), "second:%s" % kind(t["second"])] + [k for k in ("depth_tie", "sep_tie") if t[k]]
            marks += ["clamped"] * bool(t.get("clamped")) + ["rejected"] * bool(t["rejected"])
        for m in marks:
            seen.setdefault(m, set()).add(order)
    both = {"b1", "b2"}
    for m in ("ref:A", "ref:B", "ref:None", "kept:1", "kept:2", "clip:lo:p1", "clip:hi:p0", "ab_tie", "face_tie", "inc_tie", "touch",
              "sides:3+8", "sides:4+8", "box", "polygons",
              "region:inside", "region:face", "region:vertex_lo", "region:vertex_hi", "region:None", "tie", "t0", "tee",
              "first:end", "first:vertex", "first:None", "second:end", "second:vertex", "second:None", "depth_tie", "sep_tie", "clamped", "rejected"):
        assert seen.get(m) == both, "%s: reached in %s" % (m, seen.get(m))


def _equal(lib, c):
    n_lib, p_lib = debug_update_manifold_polygons(lib, c.b1, c.k1, c.p1, c.b2, c.k2, c.p2, c.count, c.pts)
    n_spec, p_spec = spec.update_manifold(c.b1, c.k1, c.p1, c.b2, c.k2, c.p2, c.count, c.pts)
    assert n_lib == n_spec, "%s: the library stores %d points, the spec %d" % (c.name, n_lib, n_spec)
    assert p_lib.tobytes() == p_spec.tobytes(), "%s: the slots differ\n%s\n%s" % (c.name, p_lib, p_spec)
    return n_spec, p_spec


def test_host_narrowphase_equals_the_spec(built_lib, cases):
    """Every case: the point count and both slots, byte for byte; and the count and the new marks the case claims."""
    for c in cases:
        n, p = _equal(built_lib, c)
        assert n == c.expect[0], "%s: %d points, the case claims %d" % (c.name, n, c.expect[0])
        assert tuple(int(v) for v in p["is_newly_created"][:n]) == tuple(c.expect[1]), c.name


def _random_pairs(seed, count):
    """Random touching pairs over all kinds with at least one polygon, in the corpus's Case form."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        bodies = []
        for _ in range(2):
            kind = int(rng.integers(0, 4))
            angle = float(rng.uniform(-np.pi, np.pi))
            pos = (float(rng.uniform(-6, 6)), float(rng.uniform(-6, 6)))
            if kind == spec.POLYGON:
                n = int(rng.integers(3, 9))
                a = np.sort(rng.uniform(0, 2 * np.pi, n))
                p = spec.polygon(np.stack([np.cos(a), np.sin(a)], axis=1) * rng.uniform(2, 6))
                if not spec.poly_valid(p):
                    break
                bodies.append(pc.poly(p, pos, angle))
            elif kind == spec.CIRCLE:
                r = float(rng.uniform(1, 4))
                bodies.append(kc.body(kind, pos, (r, r), angle))
            else:
                hy = float(rng.uniform(1, 3))
                bodies.append(kc.body(kind, pos, (hy + float(rng.uniform(0.5, 4)), hy), angle))
        if len(bodies) < 2 or spec.POLYGON not in (bodies[0]["kind"], bodies[1]["kind"]):
            continue
        a, b = bodies
        out.append(pc.Case("random%d" % len(out), "random", kc.place(a, "_t"), a["kind"], a.get("poly"), kc.place(b, "_t"), b["kind"], b.get("poly"), None, {}))
    return out


def test_host_narrowphase_equals_the_spec_on_random_pairs(built_lib):
    touching = 0
    for c in _random_pairs(7, 300):
        n, _ = _equal(built_lib, c)
        touching += n > 0
    assert touching >= 100, "only %d of the random pairs touch" % touching


def deviations(cases):
    """group -> the worst of each measure over the group's cases (the spec's points against the judge)."""
    worst = {}
    for c in cases:
        if c.group == "cache":
            worst.setdefault(c.group, dict.fromkeys(MEASURES, 0.0))
            continue
        hits, _ = trace_of(c)
        if not hits:
            continue
        verdict = ref.judge(c.b1, c.k1, c.p1, c.b2, c.k2, c.p2)
        deepest = max(range(len(hits)), key=lambda i: float(hits[i]["depth"]))
        for i, h in enumerate(hits):
            d = ref.deviation(verdict, h["p1"], h["p2"], h["n"], deepest=i == deepest)
            if i != deepest and c.group == "capsule/polygon":               # (a second candidate has its own normal: capsule_corpus)
                d["normal"] = 0.0
            w = worst.setdefault(c.group, dict.fromkeys(MEASURES, 0.0))
            for m in MEASURES:
                if d[m] > w[m]:
                    w[m] = d[m]
                    w[m + "_at"] = c.name
    return worst


def test_spec_against_the_float64_judge(cases):
    worst = deviations(cases)
    for group, figures in pc.MEASURED.items():
        for m, measured in zip(MEASURES, figures):
            bound = pc.FACTOR * max(measured, pc.FLOOR)
            print("%-18s %-8s %.3g (bound %.3g) %s" % (group, m, worst[group][m], bound, worst[group].get(m + "_at", "")))
            assert worst[group][m] <= bound, "%s %s: %.3g at %s, the bound is %.3g" % (group, m, worst[group][m], worst[group].get(m + "_at"), bound)


def test_judge_claims_every_case(cases):
    """Every case with a point gets a verdict with a depth and an axis, and the judge agrees on who touches: a pair the spec gives a
    point is not apart by more than rounding, a pair it gives none is not overlapping by more than rounding."""
    for c in cases:
        if c.group == "cache":
            continue
        hits, _ = trace_of(c)
        verdict = ref.judge(c.b1, c.k1, c.p1, c.b2, c.k2, c.p2)
        assert verdict["axes"], c.name
        tol = 1e-5
        if hits:
            assert verdict["depth"] >= -tol, "%s: the spec finds a point, the judge a gap of %g" % (c.name, -verdict["depth"])
        else:
            assert verdict["depth"] <= tol, "%s: the spec finds no point, the judge an overlap of %g" % (c.name, verdict["depth"])


def test_pairs_without_a_polygon_equal_the_plain_entry(built_lib):
    cs = [c for c in kc.cases()]
    assert len(cs) > 100
    for c in cs:
        n0, p0 = debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        n1, p1 = debug_update_manifold_polygons(built_lib, c.b1, c.k1, None, c.b2, c.k2, None, c.count, c.pts)
        assert (n0, p0.tobytes()) == (n1, p1.tobytes()), c.name
    import circle_corpus
    for c in circle_corpus.cases():
        n0, p0 = debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        n1, p1 = debug_update_manifold_polygons(built_lib, c.b1, c.k1, None, c.b2, c.k2, None, c.count, c.pts)
        assert (n0, p0.tobytes()) == (n1, p1.tobytes()), c.name


def test_debug_entry_refusals(built_lib):
    c = pc.cases()[0]
    r1, r2 = np.array([c.b1], dtype=rigid_body_dtype), np.array([c.b2], dtype=rigid_body_dtype)
    m = np.zeros(1, dtype=manifold_dtype)
    p = np.array(c.pts, dtype=contact_point_dtype)
    q = np.array([pc.SQUARE], dtype=spec.polygon_dtype)
    f = built_lib.phx_debug_update_manifold_polygons
    assert f(_ptr(r1), 3, None, _ptr(r2), 0, None, _ptr(m), _ptr(p)) != 0, "a polygon body without its polygon"
    assert f(_ptr(r1), 4, _ptr(q), _ptr(r2), 0, None, _ptr(m), _ptr(p)) != 0, "kind 4"
    bad = q.copy()
    bad["count"] = 9
    assert f(_ptr(r1), 3, _ptr(bad), _ptr(r2), 0, None, _ptr(m), _ptr(p)) != 0, "nine vertices"
    assert f(_ptr(r1), 3, _ptr(q), _ptr(r2), 0, None, _ptr(m), _ptr(p)) == 0


def test_validity():
    ok = [pc.GROUND, pc.SQUARE, pc.DIAMOND, pc.TRIANGLE, pc.OCTAGON, spec.regular(3, 1.0), spec.regular(8, 100.0)]
    assert all(spec.poly_valid(p) for p in ok)
    sq = np.array([(-4, -4), (4, -4), (4, 4), (-4, 4)], dtype=np.float64)
    bad = {
        "two vertices": spec.polygon(sq[:2]),
        "nine vertices": np.array((9, np.zeros((8, 2))), dtype=spec.polygon_dtype),
        "clockwise": spec.polygon(sq[::-1]),
        "collinear": spec.polygon([(-4, -4), (0, -4), (4, -4), (4, 4), (-4, 4)]),
        "concave": spec.polygon([(-4, -4), (4, -4), (1, 0), (4, 4), (-4, 4)]),
        "origin outside": spec.polygon(sq + 5.0),
        "origin on an edge": spec.polygon(sq + (4.0, 0.0)),
        "origin on a vertex": spec.polygon(sq + (4.0, 4.0)),
        "nan": spec.polygon([(-4, -4), (4, np.nan), (4, 4), (-4, 4)]),
        "inf": spec.polygon([(-4, -4), (np.inf, -4), (4, 4), (-4, 4)]),
        "repeated vertex": spec.polygon([(-4, -4), (4, -4), (4, -4), (4, 4), (-4, 4)]),
    }
    for why, p in bad.items():
        assert not spec.poly_valid(p), why
    assert spec.frame_box(pc.GROUND) == (F(12), F(3)) and spec.frame_box(pc.TRIANGLE) == (F(6), F(6))
    n = spec.normals(4, pc.SQUARE["v"])
    assert n[:4].tolist() == [[0, -1], [1, 0], [0, 1], [-1, 0]] and not n[4:].any()


def test_mass_helper():
    """A rectangle's corners give AddBody's box formula, a regular octagon its analytic value; the helper is the spec's."""
    hx, hy = 5.0, 3.0
    box = [(-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy)]
    m = polygon_inverse_masses(box)
    mass = 1e-5 * hx * hy
    assert m.dtype == np.float32 and m.shape == (2,)
    assert m.tolist() == [float(F(1.0) / F(mass)), float(F(1.0) / F(mass * (hx * hx + hy * hy)))]
    R = 4.0
    octagon = spec.regular(8, R)["v"].astype(np.float64)
    A = 2.0 * np.sqrt(2.0) * R * R                                          # n/2 R^2 sin(2 pi / n)
    J_over_A = R * R / 6.0 * (2.0 + np.cos(np.pi / 4.0))                    # the polar second moment of a regular n-gon per area
    mass = 1e-5 * A / 4.0
    m = polygon_inverse_masses(octagon)
    assert np.allclose(m, [1.0 / mass, 1.0 / (3.0 * mass * J_over_A)], rtol=1e-6, atol=0.0)
    assert tuple(polygon_inverse_masses(box)) == spec.masses(box)


# ---- the queries: the spec's point and ray rules against the judge on aimed random queries ----------------------------------------------
def _query_world(seed):
    """A few polygons of every vertex count, turned and placed at world scale, as records with their AABBs."""
    rng = np.random.default_rng(seed)
    recs, polys = [], []
    for n in (3, 4, 5, 6, 7, 8, 3, 8):
        a = np.sort(rng.uniform(0, 2 * np.pi, n))
        p = spec.polygon(np.stack([np.cos(a), np.sin(a)], axis=1) * rng.uniform(2, 8))
        if not spec.poly_valid(p):
            p = spec.regular(n, float(rng.uniform(2, 8)))
        b = pc.poly(p, (float(rng.uniform(-200, 200)), float(rng.uniform(-200, 200))), float(rng.uniform(-np.pi, np.pi)))
        r = kc.place(b, "")
        recs.append(r)
        polys.append(p)
    bodies = np.array(recs, dtype=rigid_body_dtype)
    for i in range(len(bodies)):                                            # UpdateGeom's AABB, as the set call leaves it
        b = bodies[i]
        dx = abs(F(b["xv"]["x"])) * F(b["geom_size"]["x"]) + abs(F(b["yv"]["x"])) * F(b["geom_size"]["y"])
        dy = abs(F(b["xv"]["y"])) * F(b["geom_size"]["x"]) + abs(F(b["yv"]["y"])) * F(b["geom_size"]["y"])
        bodies["aabb_min"]["x"][i], bodies["aabb_min"]["y"][i] = F(b["pos"]["x"]) - dx, F(b["pos"]["y"]) - dy
        bodies["aabb_max"]["x"][i], bodies["aabb_max"]["y"][i] = F(b["pos"]["x"]) + dx, F(b["pos"]["y"]) + dy
        bodies["inv_mass"][i] = bodies["inv_inertia"][i] = 1.0
    return bodies, polys


def _unit(body, *points):
    """u = 2^-24 times the scale of what the query touches: the body's position and size and the query's own points."""
    return 2.0 ** -24 * max([1.0, float(np.abs(body.pos).max()), float(body.h.max())] + [float(np.abs(np.asarray(p, dtype=np.float64)).max()) for p in points])


def test_point_rule_against_the_judge():
    bodies, polys = _query_world(3)
    kinds = np.full(len(bodies), spec.POLYGON)
    rng = np.random.default_rng(4)
    judged = grazing = 0
    for b in range(len(bodies)):
        body = ref.Body(bodies[b], spec.POLYGON, polys[b])
        centre = np.array([bodies["pos"]["x"][b], bodies["pos"]["y"][b]], dtype=np.float64)
        reach = float(np.hypot(*bodies["geom_size"][b].tolist()))
        pts = (centre + rng.uniform(-1.2 * reach, 1.2 * reach, (60, 2))).astype(F)
        got = spec.query_points(bodies[b:b + 1], kinds[b:b + 1], polys[b:b + 1], pts)
        for p, g in zip(pts, got):
            inside, d = ref.inside(body, p.astype(np.float64))
            if abs(d) < qc.NEAR * _unit(body, p):
                grazing += 1
                continue
            judged += 1
            assert (g == 0) == inside, "body %d, point %s: the spec says %s, the judge %s (distance %g)" % (b, p, g == 0, inside, d)
    print("points: %d judged, excluded share %.4f" % (judged, grazing / (judged + grazing)))
    assert judged >= 400 and grazing <= qc.CAP * (judged + grazing), (judged, grazing)


def test_ray_rule_against_the_judge():
    bodies, polys = _query_world(5)
    kinds = np.full(len(bodies), spec.POLYGON)
    rng = np.random.default_rng(6)
    judged = grazing = hits = 0
    worst = 0.0
    for b in range(len(bodies)):
        body = ref.Body(bodies[b], spec.POLYGON, polys[b])
        centre = np.array([bodies["pos"]["x"][b], bodies["pos"]["y"][b]], dtype=np.float64)
        reach = float(np.hypot(*bodies["geom_size"][b].tolist()))
        for _ in range(40):
            a = rng.uniform(0, 2 * np.pi)
            o = centre + 3.0 * reach * np.array([np.cos(a), np.sin(a)])
            target = centre + rng.uniform(-1.1 * reach, 1.1 * reach, 2)      # aimed at the body or just past it
            d = (target - o) / np.hypot(*(target - o))
            ray = np.array([o[0], o[1], d[0], d[1], 6.0 * reach], dtype=F)
            got = spec.raycast(bodies[b:b + 1], kinds[b:b + 1], polys[b:b + 1], ray.reshape(1, 5))[0]
            t, clear = ref.entry(body, ray[:2].astype(np.float64), ray[2:4].astype(np.float64), float(ray[4]))
            u = _unit(body, ray[:2], ray[:2].astype(np.float64) + float(ray[4]) * ray[2:4].astype(np.float64))
            if abs(clear) < qc.NEAR * u:
                grazing += 1
                continue
            judged += 1
            assert (got["body"] == 0) == (t is not None), "body %d, ray %s: the spec says %s, the judge %s (clearance %g)" % (b, ray, got["body"], t, clear)
            if t is None:
                continue
            hits += 1
            hit_at = ray[:2].astype(np.float64) + np.float64(got["t"]) * ray[2:4].astype(np.float64)
            worst = max(worst, abs(body.signed_distance(hit_at)) / u)
            corner = min(float(np.hypot(*(hit_at - w))) for w in body.outline)
            if corner > 1e-3 * reach:                                           # (at a corner two edges enter at once: either normal)
                n = ref.edge_normal(body, hit_at)
                assert abs(float(got["normal"][0]) - n[0]) <= 1e-5 and abs(float(got["normal"][1]) - n[1]) <= 1e-5, (b, ray, got["normal"], n)
    print("rays: %d judged, %d hits, excluded share %.4f, the hit point's distance from the surface, worst in u: %.2f" % (judged, hits, grazing / (judged + grazing), worst))
    assert worst <= qc.BOUND
    assert judged >= 250 and hits >= 150 and grazing <= qc.CAP * (judged + grazing), (judged, hits, grazing)


def test_points_and_rays_by_hand():
    """The triangle (-6,-3), (6,-3), (0,6) at (10, 5), unturned: what a frame box would contain and the triangle does not."""
    b = np.array([kc.place(pc.poly(pc.TRIANGLE, (-10.0, 15.0)), "")], dtype=rigid_body_dtype)      # (the corpus places at its origin (20, -10))
    b["aabb_min"]["x"], b["aabb_min"]["y"], b["aabb_max"]["x"], b["aabb_max"]["y"] = 4.0, -1.0, 16.0, 11.0
    b["inv_mass"] = b["inv_inertia"] = 1.0
    pts = [(10.0, 5.0), (10.0, 2.0), (10.0, 10.9), (15.0, 10.0), (4.5, 2.1), (12.9, 6.5), (13.1, 6.5), (10.0, 1.9)]
    # centre; on the bottom edge (closed); under the tip; the frame box's corner; by the bottom-left vertex; inside the right slope; outside it; below
    assert spec.query_points(b, [3], [pc.TRIANGLE], pts).tolist() == [0, 0, 0, -1, 0, 0, -1, -1]
    assert spec.query_points(b, [0], [spec.NONE], pts).tolist() == [0] * 8, "the same body as a box contains all of them"
    rays = [(13.0, 20.0, 0.0, -1.0, 100.0), (10.0, -10.0, 0.0, 1.0, 100.0), (10.0, 5.0, 1.0, 0.0, 100.0), (15.5, 20.0, 0.0, -1.0, 16.0), (30.0, 8.0, -1.0, 0.0, 100.0)]
    got = spec.raycast(b, [3], [pc.TRIANGLE], rays)
    assert got["body"].tolist() == [0, 0, 0, -1, 0]
    assert np.isclose(got["t"][0], 13.5, atol=1e-5) and got["t"].tolist()[1:3] == [12.0, 0.0] and got["normal"][2].tolist() == [0.0, 0.0]
    slope = np.array([9.0, 6.0]) / np.hypot(9.0, 6.0)
    assert np.allclose(got["normal"][0], slope, atol=1e-6) and got["normal"][1].tolist() == [0.0, -1.0]
    assert np.allclose(got["normal"][4], slope, atol=1e-6) and np.isclose(got["t"][4], 30.0 - (10.0 + 6.0 * (1.0 - 6.0 / 9.0)), atol=1e-5)
