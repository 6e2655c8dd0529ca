"""Round bodies on the CPU (include/phyx_amd.h SHAPES): phx_debug_update_manifold — the host instantiation of the narrowphase function the
device kernel calls — against tests/circle_spec.py byte for byte on the directed corpus (tests/circle_corpus.py), the corpus's claims,
the spec against its float64 judge (tests/circle_reference.py), the spec's state transforms, and the disc predicates of the queries
on hand-checked cases."""
import ctypes as C

import numpy as np
import pytest

import circle_corpus as cc
import circle_reference as ref
import circle_spec as spec
import query_corpus as qc
import query_spec
from phyx_amd.api import contact_point_dtype, manifold_dtype, rigid_body_dtype, circle_inverse_masses

F = np.float32
MEASURES = ("length", "normal", "depth", "surface")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def debug_update_manifold(lib, b1, k1, b2, k2, count, pts):
    """(point_count, pts) after phx_debug_update_manifold."""
    r1, r2 = np.array([b1], dtype=rigid_body_dtype), np.array([b2], dtype=rigid_body_dtype)
    m = np.zeros(1, dtype=manifold_dtype)
    m["body1"], m["body2"], m["point_count"], m["point_index"] = 0, 1, count, 0
    p = np.array(pts, dtype=contact_point_dtype).copy()
    assert lib.phx_debug_update_manifold(_ptr(r1), int(k1), _ptr(r2), int(k2), _ptr(m), _ptr(p)) == 0, lib.phx_last_error()
    assert (m["body1"][0], m["body2"][0], m["point_index"][0]) == (0, 1, 0)
    return int(m["point_count"][0]), p


def arm_of(c):
    """The branch case c's new point comes from, by the spec's own float32 comparisons."""
    b1, b2 = spec.Body(c.b1, c.k1), spec.Body(c.b2, c.k2)
    if c.k1 == spec.CIRCLE and c.k2 == spec.CIRCLE:
        dx, dy = b1.px - b2.px, b1.py - b2.py
        l2, R = dx * dx + dy * dy, b1.hx + b2.hx
        return "cc_miss" if l2 > R * R else ("cc" if np.sqrt(l2) > 0 else "cc_centre")
    o, b = (b1, b2) if c.k1 == spec.CIRCLE else (b2, b1)
    cx, cy = o.px - b.px, o.py - b.py
    u, v = cx * b.xvx + cy * b.xvy, cx * b.yvx + cy * b.yvy
    out_u, out_v = abs(u) > b.hx, abs(v) > b.hy
    if not out_u and not out_v:
        pu, pv = b.hx - abs(u), b.hy - abs(v)
        if abs(u) == b.hx or abs(v) == b.hy:
            return "on_face"
        return "in_tie" if pu == pv else ("in_x" if pu < pv else "in_y")
    qu = np.clip(u, -b.hx, b.hx)
    qv = np.clip(v, -b.hy, b.hy)
    ex, ey = u - qu, v - qv
    if ex * ex + ey * ey > o.hx * o.hx:
        return "miss"
    return "corner" if out_u and out_v else "face"


@pytest.fixture(scope="module")
def cases():
    return cc.cases()


def test_corpus_reaches_every_arm(cases):
    names = [c.name for c in cases]
    assert len(names) == len(set(names))
    arms = {}
    for c in cases:
        assert arm_of(c) == c.arm, c.name
        arms.setdefault(c.arm, []).append(c)
    assert set(arms) == {"cc", "cc_miss", "cc_centre", "face", "corner", "miss", "in_x", "in_y", "in_tie", "on_face"}
    for arm in ("face", "corner", "miss", "in_x", "in_y", "in_tie", "on_face"):
        first = [c for c in arms[arm] if c.k1 == spec.CIRCLE and c.group == "circle/box"]
        second = [c for c in arms[arm] if c.k2 == spec.CIRCLE and c.group == "circle/box"]
        assert first and second, "arm %s lacks a body order" % arm
        assert {c.name.replace("_b2", "")[-2:] for c in first} >= {"_q"}, "arm %s never meets a turned box" % arm


def test_host_narrowphase_equals_the_spec(built_lib, cases):
    """Every case: the point count and both slots, byte for byte; and the claim the case is named for."""
    for c in cases:
        n_lib, p_lib = debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        n_spec, p_spec = spec.update_manifold(c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        assert n_lib == n_spec, c.name
        assert p_lib.tobytes() == p_spec.tobytes(), "%s: %s != %s" % (c.name, p_lib, p_spec)
        assert n_lib == c.expect[0], c.name
        if n_lib:
            assert p_lib["is_merged"][0] == 1 and p_lib["is_newly_created"][0] == c.expect[1], c.name


def test_cache_cases(built_lib, cases):
    by = {c.name: c for c in cases}
    n, p = debug_update_manifold(built_lib, *[getattr(by["cache_matched"], k) for k in ("b1", "k1", "b2", "k2", "count", "pts")])
    assert n == 1 and p["solver_index"][0] == 7 and p["pad"][0].tolist() == [3, 9] and (p["is_merged"][0], p["is_newly_created"][0]) == (1, 0)
    assert (p["delta1"][0]["x"], p["delta1"][0]["y"], p["delta2"][0]["x"], p["delta2"][0]["y"]) == (-4.0, 0.0, 5.0, 1.0)
    assert (p["normal"][0]["x"], p["normal"][0]["y"]) == (1.0, 0.0)
    n, p = debug_update_manifold(built_lib, *[getattr(by["cache_far"], k) for k in ("b1", "k1", "b2", "k2", "count", "pts")])
    assert n == 1 and p["solver_index"][0] == -1 and (p["is_merged"][0], p["is_newly_created"][0]) == (1, 1)
    c = by["cache_box_past"]
    n, p = debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
    assert n == 1 and p["solver_index"][0] == 7, "the nearer of the two cached points survives, in slot 0"
    assert p[1].tobytes() == c.pts[1].tobytes(), "slot 1 is not written"
    c = by["cache_two_far"]
    n, p = debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
    assert n == 1 and p["solver_index"][0] == -1 and p["is_newly_created"][0] == 1
    c = by["cache_dropped"]
    n, p = debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
    assert n == 0 and p.tobytes() == c.pts.tobytes()


def test_boxes_take_the_box_path(built_lib):
    """Two boxes through the same entry: the reference's two-point face contact, which no round routine makes."""
    a, b = cc.record((0.0, 4.5), (5.0, 2.5)), cc.record((0.0, 0.0), (20.0, 2.5))
    n, p = debug_update_manifold(built_lib, a, 0, b, 0, 0, cc.blank_points())
    assert n == 2 and (p["is_newly_created"] == 1).all()
    n1, _ = debug_update_manifold(built_lib, cc.record((0.0, 4.5), (2.5, 2.5)), 1, b, 0, 0, cc.blank_points())
    assert n1 == 1


def measured(cases):
    worst = {}
    for c in cases:
        n, p = spec.update_manifold(c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        verdict = ref.judge(c.b1, c.k1, c.b2, c.k2)
        if not n:
            assert verdict["depth"] < 1e-5 * ref.scale(*verdict["bodies"]), "%s: the judge sees a penetration the spec does not" % c.name
            continue
        q = p[0]
        p1 = (np.float64(q["delta1"]["x"]) + np.float64(c.b1["pos"]["x"]), np.float64(q["delta1"]["y"]) + np.float64(c.b1["pos"]["y"]))
        p2 = (np.float64(q["delta2"]["x"]) + np.float64(c.b2["pos"]["x"]), np.float64(q["delta2"]["y"]) + np.float64(c.b2["pos"]["y"]))
        dev = ref.deviation(verdict, p1, p2, (q["normal"]["x"], q["normal"]["y"]))
        w = worst.setdefault(c.group, {"cases": 0, **{k: 0.0 for k in MEASURES}, "at": {}})
        w["cases"] += 1
        for k in MEASURES:
            if dev[k] >= w[k]:
                w[k], w["at"][k] = dev[k], c.name
    return worst


def test_spec_against_the_float64_judge(cases):
    worst = measured(cases)
    print("  group            cases     length     normal      depth    surface")
    for g, w in worst.items():
        print("  %-15s %6d %10.3g %10.3g %10.3g %10.3g" % (g, w["cases"], w["length"], w["normal"], w["depth"], w["surface"]))
    assert set(worst) == set(cc.MEASURED)
    for g, w in worst.items():
        for k, figure in zip(MEASURES, cc.MEASURED[g]):
            bound = cc.FACTOR * max(figure, cc.FLOOR)
            assert w[k] <= bound, "%s %s: %.3g at %s, the bound is %.3g" % (g, k, w[k], w["at"][k], bound)


# ---- the state transforms ----------------------------------------------------------------------------------------------------------------
def test_spec_transforms():
    kinds = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    assert spec.spawn(kinds, 2).tolist() == [0, 1, 0, 1, 1, 0, 0]
    assert spec.remove(kinds, [True, False, True, True, False]).tolist() == [0, 0, 1]
    assert spec.set_state(3).tolist() == [0, 0, 0]
    ok = spec.valid([0, 1, 1, 2, -1, 0, 0, 1, 0], [1, 2, 2, 1, 1, 0, np.inf, np.nan, 1], [2, 2, 3, 1, 1, 1, 1, np.nan, -1])
    assert ok.tolist() == [True, True, False, False, False, False, False, False, False]
    bodies = np.array([cc.record((0, 0), (2, 3)), cc.record((1, 1), (4, 4))], dtype=rigid_body_dtype)
    s = spec.shapes(bodies, [0, 1])
    assert s["kind"].tolist() == [0, 1] and s["hx"].tolist() == [2, 4] and s["hy"].tolist() == [3, 4]


def test_circle_masses_follow_add_body_scale():
    """The circle formula on AddBody's scale: mass = 1e-5f * 0.785398f * r * r, inertia = mass * 1.5f * r * r, in float32."""
    im, ii = spec.circle_masses(4.0)
    got = circle_inverse_masses([4.0, 6.0])
    assert got.dtype == np.float32 and got[0].tolist() == [float(im), float(ii)]
    assert abs(1.0 / float(im) - 1e-5 * np.pi / 4 * 16) < 1e-9
    box_mass = 1e-5 * 16
    assert abs((1.0 / float(im)) / box_mass - np.pi / 4) < 1e-6, "a quarter of the area, as for boxes"
    true_over_box = (1.0 / float(ii)) / (1.0 / float(im)) / 16
    assert abs(true_over_box - 1.5) < 1e-6, "three times the true disc inertia m r^2 / 2, as a box has three times its own"


# ---- the disc predicates on hand-checked cases ---------------------------------------------------------------------------------------------
def _disc(pos=(10.0, 5.0), r=2.0):
    b = np.array([cc.record(pos, (r, r))], dtype=rigid_body_dtype)
    b["aabb_min"]["x"], b["aabb_min"]["y"] = pos[0] - r, pos[1] - r
    b["aabb_max"]["x"], b["aabb_max"]["y"] = pos[0] + r, pos[1] + r
    b["inv_mass"], b["inv_inertia"] = 1.0, 1.0
    return b


def test_point_in_disc_by_hand():
    b = _disc()
    pts = [(10.0, 5.0), (12.0, 5.0), (11.5, 6.5), (11.0, 6.0), (12.0001, 5.0), (8.0, 3.0)]
    # centre; on the rim; inside the frame square and outside the disc (1.5^2 + 1.5^2 > 4); inside; outside the AABB; the square's corner
    assert spec.query_points(b, [1], pts).tolist() == [0, 0, -1, 0, -1, -1]
    assert spec.query_points(b, [0], pts).tolist() == [0, 0, 0, 0, -1, 0], "the same body as a box contains its corners"


def test_ray_against_disc_by_hand():
    b = _disc()
    rays = [(0.0, 5.0, 1.0, 0.0, 100.0),      # through the centre: enters at x = 8
            (0.0, 7.0, 1.0, 0.0, 100.0),      # tangent at the top (10, 7): D == 0, one root
            (10.5, 5.0, 1.0, 0.0, 100.0),     # the origin inside the disc
            (0.0, 5.0, -1.0, 0.0, 100.0),     # pointing away
            (0.0, 5.0, 1.0, 0.0, 7.5),        # max_t short of the disc
            (0.0, 6.9, 1.0, 0.0, 100.0),      # crosses the frame square near its top edge: a chord of the disc close to the tangent
            (7.0, 8.0, 1.0, -1.0, 100.0),     # diagonal, through the centre
            (8.0, 7.5, 1.0, 0.0, 100.0)]      # above the disc, outside the AABB
    h = spec.raycast(b, [1], rays)
    assert h["body"].tolist() == [0, 0, 0, -1, -1, 0, 0, -1]
    assert h["t"][0] == 8.0 and h["normal"][0].tolist() == [-1.0, 0.0] and h["point"][0].tolist() == [8.0, 5.0]
    assert h["t"][1] == 10.0 and h["normal"][1].tolist() == [0.0, 1.0] and h["point"][1].tolist() == [10.0, 7.0]
    assert h["t"][2] == 0.0 and h["normal"][2].tolist() == [0.0, 0.0] and h["point"][2].tolist() == [10.5, 5.0]
    corner = spec.raycast(b, [1], [(10.6, 8.0, 1.0, -1.0, 100.0)])      # clips the square's corner (12, 7) region and misses the disc
    assert corner["body"].tolist() == [-1]
    assert spec.raycast(b, [0], [(10.6, 8.0, 1.0, -1.0, 100.0)])["body"].tolist() == [0], "the same body as a box is hit at its corner"
    for k in range(len(rays)):
        if h["body"][k] == 0 and h["t"][k] > 0:
            n = h["normal"][k].astype(np.float64)
            assert abs(np.hypot(*n) - 1.0) < 1e-6
            assert abs(np.hypot(*(h["point"][k].astype(np.float64) - (10.0, 5.0))) - 2.0) < 1e-5


# ---- the disc predicates against the float64 judge -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in qc.cases()])
def test_spec_queries_against_the_float64_judge(name):
    """A corpus case (tests/query_corpus.py: discs and boxes, rays from 1 to 10^6 units away, bodies out to 10^5), circle_spec against
    the float64 judge (tests/query_reference.py):
      - every (ray, body) and (point, body) pair: the rule's verdict is the judge's wherever the clearance exceeds NEAR = 32 u,
        u = 2^-24 * scale; the pairs excused are at most CAP = 0.02 of the case's, by the judge alone;
      - the closest hit: the judge's body unless two entries are within 32 u, the normal (0, 0) exactly when the origin is inside, and
        every deviation() measure (hit point, normal length and angle times r, the returned point's distance from the surface) within
        BOUND = 16 u.  The ray/disc rule meets 16 at every distance (it measures under 3); only a box's `hit` has a wider bound, for
        the reason test_queries_cpu.test_spec_box_rules_against_the_float64_judge gives;
      - the deliberately doubtful rays (grazing at 0.999 r and 1.001 r, max_t an ulp either side of the entry) and points: excused or
        right, not counted in the share.
    The quadratic this rule replaced (c = rx*rx + ry*ry - r*r, D = b*b - a*c) fails here from 30 units on: its hit point is off by 25 u
    at 30 units, 1850 u at 300 and 5500 u at 3000, from where on it also loses clear hits and returns normals of length 0."""
    c = qc.case(name)
    g = query_spec.Geometry(c.bodies)
    round_ = c.kinds == qc.CIRCLE
    ray_verdicts = lambda r: np.where(round_, spec.ray_circle(g, r)[0], query_spec.ray_box(g, r)[0]) & query_spec.ray_candidate(g, r)      # noqa: E731
    point_verdicts = lambda p: np.where(round_, spec.point_in_circle(g, p[0], p[1]), query_spec.point_in_box(g, p[0], p[1]))            # noqa: E731
    if len(c.rays):
        near = qc.judge_pairs(c.bodies, c.kinds, c.rays, ray_verdicts)
        assert near.mean() <= qc.CAP, "excluded share %.4f" % near.mean()
        _, worst = qc.judge_hits(c.bodies, c.kinds, c.rays, spec.raycast(c.bodies, c.kinds, c.rays))
        print("%s: %d rays, excluded %.4f of the pairs; worst in u: %s" % (name, len(c.rays), near.mean(), qc.table(worst)))
        qc.assert_bounds(worst, name)
    if len(c.near_rays):
        qc.judge_pairs(c.bodies, c.kinds, c.near_rays, ray_verdicts)
        qc.judge_hits(c.bodies, c.kinds, c.near_rays, spec.raycast(c.bodies, c.kinds, c.near_rays))
    if len(c.points):
        near = qc.judge_points(c.bodies, c.kinds, c.points, spec.query_points(c.bodies, c.kinds, c.points), point_verdicts)
        assert near.mean() <= qc.CAP, "excluded share of the points' pairs %.4f" % near.mean()
        qc.judge_points(c.bodies, c.kinds, c.near_points, spec.query_points(c.bodies, c.kinds, c.near_points), point_verdicts)


def test_the_rows_seen_from_3000_units_name_the_nearest_disc():
    """Six discs in a row, indices scrambled, seen along the row from 3000 units on either side: the nearest by the judge, not body 0."""
    c = qc.case("a row of discs from 3000")
    h = spec.raycast(c.bodies, c.kinds, c.rays)
    assert h["body"].tolist() == [3, 2, -1, 3, 2, -1, 3, 2, -1, 1, 2, -1]
