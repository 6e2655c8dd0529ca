"""Capsule bodies on the CPU (include/phyx_amd.h SHAPES): phx_debug_update_manifold — the host instantiation of the narrowphase function
the device kernel calls — against tests/capsule_spec.py byte for byte on the directed corpus (tests/capsule_corpus.py), the corpus's
claims, the spec against its float64 judge (tests/capsule_reference.py), the spec's state transforms, the mass formula, and the
capsule predicates of the queries against the judge."""
import numpy as np
import pytest

import capsule_corpus as kc
import capsule_reference as ref
import capsule_spec as spec
import circle_spec
import query_corpus as qc
import query_spec
import round_query_spec as rq
from phyx_amd.api import capsule_inverse_masses, circle_inverse_masses, rigid_body_dtype
from test_circles_cpu import debug_update_manifold

F = np.float32
FIRST = ("length", "normal", "depth", "surface")
SECOND = ("length", "surface", "disc", "across")


@pytest.fixture(scope="module")
def cases():
    return kc.cases()


def trace_of(c):
    b1, b2 = spec.Body(c.b1, c.k1), spec.Body(c.b2, c.k2)
    cands, t = spec.candidates(b1, b2), {}
    first, second = spec.select(cands, t)
    if first is None:
        t.update(first=None, second=None, rejected=[], sep_tie=False, depth_tie=False)
    return b1, b2, cands, t


def discs_against_capsules(b1, b2):
    """Every (name, disc centre, disc radius, capsule) the pair's candidates are made of, whether they count or not."""
    out = []
    if b1.kind == spec.CAPSULE and b2.kind == spec.CAPSULE:
        for who, a, b in (("end", b1, b2), ("other", b2, b1)):
            out += [("%s%d" % (who, i), e, a.hy, b) for i, e in enumerate(spec.ends(a))]
    elif spec.CIRCLE in (b1.kind, b2.kind):
        c, k = (b1, b2) if b1.kind == spec.CIRCLE else (b2, b1)
        out.append(("circle", (c.px, c.py), c.hx, k))
    else:
        k, b = (b1, b2) if b1.kind == spec.CAPSULE else (b2, b1)
        out += [("corner%d" % i, p, F(0), k) for i, p in enumerate(spec.corners(b))]
    return out


def holds(flag, c, b1, b2, cands, t):
    """The corpus's flag, by the spec's own float32 comparisons."""
    by_name = dict(cands)
    raw = {name: (spec.disc_capsule(p[0], p[1], r, k, True), p, k) for name, p, r, k in discs_against_capsules(b1, b2)}
    if flag in ("depth_tie", "sep_tie"):
        return t[flag]
    if flag.startswith("rejected:"):
        _, name, halves = flag.split(":")
        return (name, halves[0] == "t", halves[1] == "t") in t["rejected"]
    if flag.startswith("clamped:"):
        name = flag.split(":")[1]
        (cand, unclamped), _, _ = raw[name]
        return cand is not None and not unclamped and by_name[name] is None
    if flag == "at_end":
        (cand, unclamped), _, _ = raw["circle"]
        return cand is not None and not unclamped and by_name["circle"] is not None
    if flag == "at_a":
        def u_of(p, k):
            ex, ey = p[0] - k.px, p[1] - k.py
            return ex * k.xvx + ey * k.xvy
        return any(abs(u_of(p, k)) == spec.half(k) and by_name[name] is not None for name, ((_, _), p, k) in raw.items())
    if flag == "on_core":
        k = b2 if b1.kind == spec.CIRCLE else b1
        n = by_name["circle"]["n"]
        return (abs(n[0]), abs(n[1])) == (abs(k.yvx), abs(k.yvy)) and by_name["circle"]["depth"] == k.hy + (b1.hx if b1.kind == spec.CIRCLE else b2.hx)
    if flag == "inside":
        k, b = (b1, b2) if b1.kind == spec.CAPSULE else (b2, b1)
        for ex, ey in spec.ends(k):
            u = (ex - b.px) * b.xvx + (ey - b.py) * b.xvy
            v = (ex - b.px) * b.yvx + (ey - b.py) * b.yvy
            if abs(u) <= b.hx and abs(v) <= b.hy:
                return True
        return False
    if flag == "touch":
        return any(cand is not None and cand["depth"] == 0 for _, cand in cands)
    if flag == "near_circle":
        return any(b.kind == spec.CAPSULE and spec.half(b) == np.spacing(b.hy) for b in (b1, b2))
    if flag == "crossed":
        return ref.judge(c.b1, c.k1, c.b2, c.k2)["normal"] is None
    raise ValueError(flag)


def test_corpus_reaches_every_arm(cases):
    names = [c.name for c in cases]
    assert len(names) == len(set(names))
    firsts, seconds, flags = {}, {}, {}
    for c in cases:
        b1, b2, cands, t = trace_of(c)
        assert (t["first"], t["second"]) == (c.first, c.second), "%s: the spec selects %s, %s" % (c.name, t["first"], t["second"])
        for f in c.flags:
            assert holds(f, c, b1, b2, cands, t), "%s: %s does not hold (%s)" % (c.name, f, t)
        if c.group == "cache":
            continue
        order = "b2" if c.name.endswith("_b2") else "b1"
        turned = "_t" in c.name.replace("_b2", "")[-2:] or "_q" in c.name.replace("_b2", "")[-2:]
        kind = lambda n: None if n is None else n.rstrip("0123")      # noqa: E731
        for table, key in ((firsts, kind(c.first)), (seconds, kind(c.second))):
            table.setdefault((c.group, key), set()).update({order, "turned" if turned else "plain"})
        for f in c.flags:
            flags.setdefault(f.split(":")[0] + (":" + f.split(":")[2] if f.startswith("rejected") else ""), set()).update({order, "turned" if turned else "plain"})
    every = {"b1", "b2", "turned", "plain"}
    # every candidate kind wins first and wins second (a circle is the only candidate of its pair: it cannot come second), none at all
    for key in (("capsule/box", "end"), ("capsule/box", "corner"), ("capsule/box", None), ("capsule/circle", "circle"), ("capsule/circle", None),
                ("capsule/capsule", "end"), ("capsule/capsule", "other"), ("capsule/capsule", None)):
        assert firsts.get(key) == every, "first %s: %s" % (key, firsts.get(key))
    for key in (("capsule/box", "end"), ("capsule/box", "corner"), ("capsule/box", None), ("capsule/capsule", "end"), ("capsule/capsule", "other"),
                ("capsule/capsule", None)):
        assert seconds.get(key) == every, "second %s: %s" % (key, seconds.get(key))
    for f in ("depth_tie", "sep_tie", "rejected:ff", "rejected:tf", "rejected:ft", "clamped", "at_end", "at_a", "on_core", "inside", "touch", "near_circle", "crossed"):
        assert flags.get(f) == every, "%s: %s" % (f, flags.get(f))
    both_ends = {c.first for c in cases} | {c.second for c in cases}
    assert both_ends >= {"end0", "end1", "other0", "other1", "corner0", "corner1", "corner2", "corner3", "circle"}


def test_host_narrowphase_equals_the_spec(built_lib, cases):
    """Every case: the point count and both slots, byte for byte; and the count and the new marks the case claims."""
    for c in cases:
        n_lib, p_lib = debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        n_spec, p_spec = spec.update_manifold(c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        assert n_lib == n_spec, c.name
        assert p_lib.tobytes() == p_spec.tobytes(), "%s: %s != %s" % (c.name, p_lib, p_spec)
        assert n_lib == c.expect[0], c.name
        assert tuple(p_lib["is_newly_created"][:n_lib].tolist()) == tuple(c.expect[1]) and (p_lib["is_merged"][:n_lib] == 1).all(), c.name


def test_pairs_without_a_capsule_are_the_round_spec(built_lib):
    import circle_corpus as cc
    for c in cc.cases():
        n_spec, p_spec = spec.update_manifold(c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        n_old, p_old = circle_spec.update_manifold(c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        assert n_spec == n_old and p_spec.tobytes() == p_old.tobytes(), c.name


def _points(c, q):
    p1 = np.array([np.float64(q["delta1"]["x"]) + np.float64(c.b1["pos"]["x"]), np.float64(q["delta1"]["y"]) + np.float64(c.b1["pos"]["y"])])
    p2 = np.array([np.float64(q["delta2"]["x"]) + np.float64(c.b2["pos"]["x"]), np.float64(q["delta2"]["y"]) + np.float64(c.b2["pos"]["y"])])
    return p1, p2, np.array([np.float64(q["normal"]["x"]), np.float64(q["normal"]["y"])])


def test_the_named_claims(built_lib, cases):
    by = {c.name: c for c in cases}
    for name in ("kb_flat", "kb_flat_q", "kb_flat_b2", "kb_lean_t"):      # flat on a face: two points, one normal, at least 2a apart
        c = by[name]
        n, p = debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        assert n == 2
        (a1, a2, na), (b1, b2, nb) = _points(c, p[0]), _points(c, p[1])
        apart = 12.0 - 1e-5 if "lean" not in name else 12.0 * np.cos(0.05) - 1e-5      # (leaning by 0.05 rad, the box's points are 2a cos apart)
        if "lean" not in name:
            assert (na == nb).all()
        assert na @ nb > 0.99 and np.hypot(*(a1 - b1)) >= apart and np.hypot(*(a2 - b2)) >= apart
    for name in ("kb_on_end", "kb_on_end_t_b2", "kb_on_other_end_q", "kk_standing"):      # on end: one point
        c = by[name]
        assert debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)[0] == 1, name
    for name in ("kb_across", "kb_across_tie_q_b2", "kb_across_back_t"):      # across a narrow box: its two upper corners
        c = by[name]
        n, p = debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        assert n == 2 and {c.first, c.second} == {"corner2", "corner3"}
        box = ref.Body(c.b2, c.k2) if c.k2 == spec.BOX else ref.Body(c.b1, c.k1)
        top = [box.pos + box.xv * s * box.h[0] + box.yv * box.h[1] for s in (-1, 1)]
        on_box = [_points(c, q)[1 if c.k2 == spec.BOX else 0] for q in p]
        assert all(min(np.hypot(*(q - t)) for t in top) < 1e-5 for q in on_box)


def test_cache_cases(built_lib, cases):
    by = {c.name: c for c in cases}
    run = lambda c: debug_update_manifold(built_lib, c.b1, c.k1, c.b2, c.k2, c.count, c.pts)      # noqa: E731
    n, p = run(by["cache2_matched"])
    assert n == 2 and p["solver_index"].tolist() == [7, 8] and p["pad"].tolist() == [[3, 9], [1, 2]] and p["is_newly_created"].tolist() == [0, 0]
    assert p["delta1"]["x"].tolist() == [-6.0, 6.0] and p["delta2"]["y"].tolist() == [3.0, 3.0] and p["normal"]["y"].tolist() == [1.0, 1.0]
    n, p = run(by["cache2_far"])
    assert n == 2 and p["solver_index"].tolist() == [-1, -1] and p["delta1"]["x"].tolist() == [-6.0, 6.0]
    n, p = run(by["cache2_two_far"])
    assert n == 2 and p["solver_index"].tolist() == [-1, -1] and p["is_newly_created"].tolist() == [1, 1]
    n, p = run(by["cache2_one_matched"])
    assert n == 2 and p["solver_index"].tolist() == [8, -1] and p["delta1"]["x"].tolist() == [6.0, -6.0], "the matched cached point keeps its slot order"
    c = by["cache2_dropped"]
    n, p = run(c)
    assert n == 0 and p.tobytes() == c.pts.tobytes()


def measured(cases):
    worst = {}
    for c in cases:
        n, p = spec.update_manifold(c.b1, c.k1, c.b2, c.k2, c.count, c.pts)
        verdict = ref.judge(c.b1, c.k1, c.b2, c.k2)
        if not n:
            # (where the cores cross, the known limit, the judge has no depth: the rule is defined there and claims nothing)
            assert verdict["depth"] is None or verdict["depth"] < 1e-5 * ref.scale(*verdict["bodies"]), "%s: the judge sees a penetration the spec does not" % c.name
            assert verdict["depth"] is not None or "crossed" in c.flags, c.name
            continue
        w = worst.setdefault(c.group, {"cases": 0, "seconds": 0, "first": {k: 0.0 for k in FIRST}, "second": {k: 0.0 for k in SECOND}, "at": {}})
        # the stored order is the selection's unless a cached point was matched: the deeper point is the first
        stored = [_points(c, p[k]) for k in range(n)]
        if n == 2 and c.group == "cache" and c.expect[1] == (0, 1):
            stored.reverse()
        w["cases"] += 1
        dev = ref.deviation(verdict, *stored[0])
        for k in FIRST:
            if dev[k] >= w["first"][k]:
                w["first"][k], w["at"][k] = dev[k], c.name
        if n == 2:
            w["seconds"] += 1
            dev = ref.second(verdict, *stored[1])
            for k in SECOND:
                if dev[k] >= w["second"][k]:
                    w["second"][k], w["at"]["2:" + k] = dev[k], c.name
    return worst


def test_spec_against_the_float64_judge(cases):
    worst = measured(cases)
    print("  group            cases     length     normal      depth    surface  |  seconds     length    surface       disc     across")
    for g, w in worst.items():
        print("  %-15s %6d %10.3g %10.3g %10.3g %10.3g  | %8d %10.3g %10.3g %10.3g %10.3g" % (g, w["cases"], *[w["first"][k] for k in FIRST], w["seconds"],
                                                                                      *[w["second"][k] for k in SECOND]))
    assert set(worst) == set(kc.MEASURED)
    for g, w in worst.items():
        for which, names, figures in (("first", FIRST, kc.MEASURED[g][0]), ("second", SECOND, kc.MEASURED[g][1])):
            for k, figure in zip(names, figures):
                bound = kc.FACTOR * max(figure, kc.FLOOR)
                assert w[which][k] <= bound, "%s %s %s: %.3g at %s, the bound is %.3g" % (g, which, k, w[which][k], w["at"], bound)


# ---- the state transforms and the masses ----------------------------------------------------------------------------------------------------
def test_spec_transforms():
    kinds = np.array([0, 2, 0, 1, 2], dtype=np.int32)
    assert spec.spawn(kinds, 2).tolist() == [0, 2, 0, 1, 2, 0, 0]
    assert spec.remove(kinds, [True, False, True, True, True]).tolist() == [0, 0, 1, 2]
    assert spec.set_state(3).tolist() == [0, 0, 0]
    ok = spec.valid([2, 2, 2, 2, 2, 2, 1, 0, 3], [4, 3, 2, 4, np.inf, np.nan, 2, 1, 4], [2, 3, 3, 0, 2, 2, 2, 2, 2])
    assert ok.tolist() == [True, False, False, False, False, False, True, True, False]
    bodies = np.array([kc.record((0, 0), (4, 2)), kc.record((1, 1), (4, 4))], dtype=rigid_body_dtype)
    s = spec.shapes(bodies, [2, 1])
    assert s["kind"].tolist() == [2, 1] and s["hx"].tolist() == [4, 4] and s["hy"].tolist() == [2, 4]


def test_capsule_masses_follow_add_body_scale():
    im, ii = spec.masses(8.0, 2.0)
    got = capsule_inverse_masses([8.0, 5.0], [2.0, 1.0])
    assert got.dtype == np.float32 and got.shape == (2, 2) and got[0].tolist() == [float(im), float(ii)]
    a, r = 6.0, 2.0
    mass = 1e-5 * (a * r + np.pi / 4 * r * r)                           # a quarter of the area 4ar + pi r^2
    assert abs(1.0 / float(im) - mass) < 1e-6 * mass
    # three times the true inertia: the rectangle m (w^2 + h^2) / 12 with w = 2a, h = 2r, and the two half discs about the capsule's
    # centre, by the parallel axis theorem from the half disc's centroid at 4r / (3 pi) beyond its flat side
    true_box = (4 * a * r) * ((2 * a) ** 2 + (2 * r) ** 2) / 12.0
    c = 4 * r / (3 * np.pi)
    half = np.pi * r * r / 2
    true_caps = 2 * ((half * r * r / 2 - half * c * c) + half * (a + c) ** 2)
    assert abs(1.0 / float(ii) - 1e-5 * 3 * (true_box + true_caps) / 4) < 1e-5 * (1.0 / float(ii))
    # a -> 0: the circle formula
    for r in (0.5, 3.0, 40.0):
        near = capsule_inverse_masses(np.nextafter(F(r), F(np.inf)), r)[0]
        disc = circle_inverse_masses(r)[0]
        assert np.allclose(near, disc, rtol=1e-6, atol=0.0)


# ---- the capsule predicates against the float64 judge ---------------------------------------------------------------------------------------
QUERY_ROWS = [(0.0, 0.0, "0", 8.0, 2.0, 2), (40.0, 5.0, "pi/2", 6.0, 1.5, 2), (-30.0, 20.0, 0.6435, 10.0, 4.0, 2), (15.0, -35.0, -1.1, 3.0, 2.5, 2),
              (3000.0, 1200.0, 0.3, 9.0, 2.0, 2), (-25.0, -25.0, 2.5, 20.0, 0.5, 2)]


def _query_world():
    bodies, kinds = qc.records(QUERY_ROWS)
    return bodies, kinds, [ref.Body(b, 2) for b in bodies]


def _units(body, *points):
    return 2.0 ** -24 * max(1.0, np.abs(body.pos).max(), body.h.max(), *[np.abs(np.asarray(p, dtype=np.float64)).max() for p in points])


def _aimed_queries(rng, judges, count):
    """Points around every capsule at -0.5 .. 2.5 radii from its core, and rays from 1 .. 300 units away aimed at such points."""
    pts, rays = [], []
    for b in judges:
        a = float(b.core()[0][1] @ b.xv - b.pos @ b.xv)
        for _ in range(count):
            u, ang, rho = rng.uniform(-a, a), rng.uniform(0, 2 * np.pi), rng.uniform(0.0, 2.5) * b.radius
            core = b.pos + b.xv * u
            target = core + rho * (b.xv * np.cos(ang) + b.yv * np.sin(ang)) + (b.xv * np.sign(np.cos(ang)) * (a - abs(u)) if rng.random() < 0.4 else 0.0)
            pts.append(target)
            dist, heading = rng.choice([1.0, 10.0, 30.0, 300.0]), rng.uniform(0, 2 * np.pi)
            d = np.array([np.cos(heading), np.sin(heading)]) * rng.choice([1.0, 1e-3, 1e3])
            o = target - d / np.hypot(*d) * (dist + 3 * b.radius)
            rays.append((*o, *d, rng.choice([1.0, 0.5, 2.0]) * (dist + 3 * b.radius) / np.hypot(*d)))
    return np.array(pts, dtype=F), np.array(rays, dtype=F)


def test_spec_queries_against_the_float64_judge():
    """Every (query, capsule) pair: the rule's verdict is the judge's wherever the judge's clearance exceeds NEAR = 32 u, u = 2^-24 * scale;
    the pairs excused are at most CAP = 0.02 of each kind's, by the judge alone (the queries are drawn at random distances from the
    surfaces, so few of them lie within 32 u of one).  The closest hit of a ray or a cast, where both sides see one: the returned point
    lies within BOUND = 16 u of the capsule grown by the query's radius."""
    bodies, kinds, judges = _query_world()
    g = query_spec.Geometry(bodies)
    rng = np.random.default_rng(20260)
    pts, rays = _aimed_queries(rng, judges, 40)
    shares = {}

    def tally(kind, verdicts, clearances, scales):
        near = np.abs(clearances) < qc.NEAR * scales
        wrong = (verdicts != (clearances <= 0)) & ~near
        assert not wrong.any(), "%s: %d verdicts differ from the judge's beyond %g u" % (kind, wrong.sum(), qc.NEAR)
        shares[kind] = near.mean()
        assert near.mean() <= qc.CAP, "%s: excluded share %.4f" % (kind, near.mean())

    v = np.array([spec.point_in_capsule(g, p[0], p[1]) for p in pts])
    c = np.array([[ref.signed_distance(b, p) for b in judges] for p in pts])
    tally("points", v, c, np.array([[_units(b, p) for b in judges] for p in pts]))

    radii = rng.choice([0.5, 2.0, 6.0], size=len(pts))
    circles = np.column_stack([pts, radii]).astype(F)
    kd = np.asarray(kinds)
    v = np.array([spec.overlap(g, kd, q) for q in circles])
    c = np.array([[ref.signed_distance(b, q[:2], float(q[2])) for b in judges] for q in circles])
    tally("circles", v, c, np.array([[_units(b, q[:2]) for b in judges] for q in circles]))

    def entries(rows, grow):
        v, c, s, worst = [], [], [], 0.0
        for q, row in enumerate(rows):
            ox, oy, dx, dy, max_t = (F(x) for x in row[-5:]) if grow is None else (F(row[0]), F(row[1]), F(row[3]), F(row[4]), F(row[5]))
            r = F(0) if grow is None else F(row[2])
            hit, tin, *_ = spec.ray_capsule(g, ox - g.px, oy - g.py, dx, dy, max_t, g.hy + r if grow is not None else g.hy)
            cand = query_spec.ray_candidate(g, row) if grow is None else rq.cast_candidate(g, row)
            v.append(hit & cand)
            got = [ref.entry(b, (float(ox), float(oy)), (float(dx), float(dy)), float(max_t), float(r)) for b in judges]
            c.append([e[1] for e in got])
            end = np.array([float(ox), float(oy)]) + float(max_t) * np.array([float(dx), float(dy)])
            s.append([_units(b, (ox, oy), end) for b in judges])
            for k, (t, _) in enumerate(got):
                if t is not None and t > 0 and v[-1][k]:
                    at = np.array([np.float64(ox), np.float64(oy)]) + np.float64(max(tin[k], F(0))) * np.array([np.float64(dx), np.float64(dy)])
                    worst = max(worst, abs(ref.signed_distance(judges[k], at, float(r))) / s[-1][k])
        return np.array(v), np.array(c), np.array(s), worst

    v, c, s, worst_ray = entries(rays, None)
    tally("rays", v, c, s)
    casts = np.column_stack([rays[:, 0], rays[:, 1], rng.choice([0.5, 2.0, 6.0], size=len(rays)), rays[:, 2], rays[:, 3], rays[:, 4]]).astype(F)
    v, c, s, worst_cast = entries(casts, True)
    tally("casts", v, c, s)
    print("excluded shares: %s; the hit point's distance from the surface, worst in u: rays %.2f, casts %.2f" % (
        ", ".join("%s %.4f" % kv for kv in shares.items()), worst_ray, worst_cast))
    assert worst_ray <= qc.BOUND and worst_cast <= qc.BOUND


def test_capsule_predicates_by_hand():
    bodies, kinds = qc.records([(10.0, 5.0, "0", 6.0, 2.0, 2)])      # the core from (6, 5) to (14, 5), r = 2
    pts = [(10.0, 5.0), (10.0, 7.0), (15.9, 5.0), (15.5, 6.5), (15.5, 6.3), (4.1, 5.0), (3.9, 5.0), (10.0, 7.1)]
    # centre; on the side; in the right cap; in the frame box's corner and outside the cap (1.5^2 + 1.5^2 > 4); inside it; the left cap
    assert spec.query_points(bodies, kinds, pts).tolist() == [0, 0, 0, -1, 0, 0, -1, -1]
    assert circle_spec.query_points(bodies, [0], pts).tolist() == [0, 0, 0, 0, 0, 0, -1, -1], "the same body as a box holds its corners"
    detail = []
    rays = [(10.0, 20.0, 0.0, -1.0, 100.0),      # down onto the side: enters at y = 7
            (10.0, -20.0, 0.0, 1.0, 100.0),      # up onto the other side: y = 3
            (30.0, 5.0, -1.0, 0.0, 100.0),       # along the axis from the right: the right cap at x = 16
            (-10.0, 5.0, 1.0, 0.0, 100.0),       # ... from the left: x = 4
            (11.0, 5.5, 1.0, 0.0, 100.0),        # the origin inside
            (15.9, 20.0, 0.0, -1.0, 100.0),      # down past the side's end: the right cap
            (15.9, 20.0, 0.0, -1.0, 10.0),       # ... max_t short of it
            (16.5, 20.0, 0.0, -1.0, 100.0)]      # beside the capsule
    h = spec.raycast(bodies, kinds, rays, detail=detail)
    assert detail == ["side+", "side-", "end1", "end0", "inside", "end1", None, None]
    assert h["body"].tolist() == [0, 0, 0, 0, 0, 0, -1, -1]
    assert h["t"][:5].tolist() == [13.0, 23.0, 14.0, 14.0, 0.0]
    assert h["normal"][:5].tolist() == [[0.0, 1.0], [-0.0, -1.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 0.0]]
    assert h["point"][:4].tolist() == [[10.0, 7.0], [10.0, 3.0], [16.0, 5.0], [4.0, 5.0]]
    off, hits = spec.query_circles(bodies, kinds, [(10.0, 8.0, 1.0), (10.0, 8.1, 1.0), (17.0, 5.0, 1.0), (16.5, 7.5, 1.0), (16.5, 7.5, 1.6)])
    assert off.tolist() == [0, 1, 1, 2, 2, 3] and hits.tolist() == [0, 0, 0]
    detail = []
    c = spec.cast_circles(bodies, kinds, [(10.0, 20.0, 1.0, 0.0, -1.0, 100.0), (30.0, 5.0, 1.0, -1.0, 0.0, 100.0), (10.0, 6.0, 1.0, 1.0, 0.0, 5.0)], detail=detail)
    assert detail == ["side+", "end1", "inside"] and c["t"].tolist() == [12.0, 13.0, 0.0] and c["normal"].tolist() == [[0.0, 1.0], [1.0, 0.0], [0.0, 0.0]]
