"""A directed corpus for the nearest-body query (tests/near_reference.py is its judge), in the manner of tests/round_query_corpus.py:
small sets of boxes, circles, capsules and polygons, and points placed against each of them by construction.

What varies: for every face or edge and every corner or vertex of every body (a circle: four directions; a capsule: its sides, its
tips and obliquely off its ends) a point 1e-3, 0.5, 3 and 100 units out along the outward direction, for the first face and the first
corner of every body also 1 .. 10^6 units out (query_corpus.DISTANCES), and inside at 0.5 and 0.9 of the way from the body's position
towards each of those surface points; the centre of every circle, three points on every capsule's core and every box's centre;
bodies near the world's origin, at 3000 and at 10^5 from it; frames that include 0 and pi / 2 exactly; max_dist generous (twice the
distance out and 10 more), FLT_MAX on every third query, and just short of and past the distance; a row of bodies of all four kinds
in which the nearer body has the higher index.

A case's `queries` are the ones whose answer is clear BY DESIGN, and the judge alone decides that, before any code under test has
run: a query is put there only if, by the judge's float64 figures, every body is at least DESIGN u from max_dist or out of the
running, the runner-up is at least DESIGN u behind the winner, and the winner's foot and normal are at least DESIGN u from jumping
(inside: the medial set; outside: a corner's or a vertex's tip, where the inside's medial set meets the surface).  Every other query
goes to `near_queries`, which are only asserted "excused or right"; so do the deliberately doubtful ones: max_dist at the distance
and one ulp either way, the medial points above, a point at equal distance from two bodies.

Bounds, in u = 2^-24 * the largest of 1, |p|, |pos|, the sizes and |sd| (near_reference.unit).  Every measure starts at
query_corpus.BOUND = 16 u.  The specification's worst against the judge over the whole corpus, measured on the CPU
(tests/test_near_queries_cpu.py prints the table), as distance / point / normal / length: box 4.99 / 2.50 / 6.07 / 3.11, circle
1.58 / 0.72 / 0.15 / 1.44, capsule 3.11 / 4.60 / 4.09 / 1.24, polygon 6.16 / 0.96 / 5.70 / 4.11.  All of it is within BOUND, so no
measure has a bound of its own and BOUNDS is empty (Queries: nearest)."""
import functools

import numpy as np

import near_reference as ref
import polygon_spec as ps
import query_corpus as qc
from query_corpus import BOUND, CAP, DESIGN, DISTANCES, NEAR, judged, records      # noqa: F401

F = np.float32
BOX, CIRCLE, CAPSULE, POLYGON = 0, 1, 2, 3
FLT_MAX = float(np.finfo(F).max)
OUTS = (1e-3, 0.5, 3.0, 100.0)
INSIDE = (0.5, 0.9)
# Measures that exceed BOUND, each with the term that causes it (the precedent of round_query_corpus.BOUNDS); empty: none does.
BOUNDS = {}


def polygons():
    """The corpus's four polygons: a scalene triangle, a regular pentagon, a stretched octagon, a thin quadrilateral."""
    octagon = np.asarray(ps.regular(8, 6.0, 0.2)["v"], dtype=np.float64) * (1.5, 1.0)
    return [ps.polygon([(-2.0, -1.0), (3.0, -1.0), (0.0, 2.5)]), ps.regular(5, 4.0, 0.3), ps.polygon(octagon),
            ps.polygon([(-10.0, -0.5), (10.0, -0.5), (10.0, 0.5), (-10.0, 0.5)])]


def near_set(shift=(0.0, 0.0)):
    """Four boxes, three circles, four capsules and four polygons near a grid 90 apart around `shift`: (rows, polys), rows as
    query_corpus.records takes them, polys a list with a phx_polygon (polygon_spec) where the kind is a polygon, None elsewhere."""
    shapes = [(BOX, 0.5, 0.5, "0"), (CIRCLE, 0.5, 0.5, "0"), (CAPSULE, 3.0, 1.0, "0"), (POLYGON, 0, 0, 0.262),
              (BOX, 5.0, 2.0, 0.262), (CIRCLE, 2.0, 2.0, 1.0), (CAPSULE, 12.0, 0.5, 2.827), (POLYGON, 1, 0, "0"),
              (BOX, 20.0, 8.0, "pi/2"), (CIRCLE, 8.0, 8.0, "pi/2"), (CAPSULE, 6.0, 4.0, "pi/2"), (POLYGON, 2, 0, "pi/2"),
              (BOX, 3.0, 3.0, 4.189), (CAPSULE, 2.0, 1.5, -1e-3), (POLYGON, 3, 0, 5.0)]
    spots = [(x, y) for y in (-90.0, 0.0, 90.0) for x in (-180.0, -90.0, 0.0, 90.0, 180.0)]
    gons = polygons()
    rows, polys = [], []
    for i, ((kind, hx, hy, ang), (x, y)) in enumerate(zip(shapes, spots)):
        x, y = x + 1.7 * ((i * 7) % 5) + shift[0], y + 2.3 * ((i * 3) % 7) + shift[1]      # (off the grid, as query_corpus.small_set)
        poly = None
        if kind == POLYGON:
            poly = gons[int(hx)]
            hx, hy = (float(v) for v in ps.frame_box(poly))
        rows.append((x, y, ang, hx, hy, kind))
        polys.append(poly)
    return rows, polys


def row_set():
    """Bodies of all four kinds in a row along x, 14 apart, the index order scrambled: beside most of them the nearest is not body 0."""
    xs = (42.0, 14.0, 70.0, 0.0, 28.0, 56.0)
    kinds = (CIRCLE, BOX, CAPSULE, POLYGON, CIRCLE, BOX)
    gons = polygons()
    rows, polys = [], []
    for i, (x, kind) in enumerate(zip(xs, kinds)):
        poly = gons[0] if kind == POLYGON else None
        hx, hy = (float(v) for v in ps.frame_box(poly)) if poly is not None else ((2.0, 1.0) if kind == CAPSULE else (1.0 + 0.25 * i, 1.0 + 0.25 * i))
        rows.append((x, 0.0, "0" if i % 2 else 0.3, hx, hy, kind))
        polys.append(poly)
    return rows, polys


def world(bodies, kinds, polys):
    """A device world that holds the records' bodies: query_corpus.world for the boxes and circles, then set_shapes for the capsules
    and set_polygons for the polygons; no step."""
    import phyx_amd
    kinds = np.asarray(kinds)
    w = qc.world(bodies, np.where(kinds == CIRCLE, CIRCLE, BOX))
    caps = np.flatnonzero(kinds == CAPSULE).astype(np.int32)
    if len(caps):
        w.set_shapes(caps, phyx_amd.SHAPE_CAPSULE, bodies["geom_size"]["x"][caps], bodies["geom_size"]["y"][caps])
    gons = np.flatnonzero(kinds == POLYGON).astype(np.int32)
    if len(gons):
        w.set_polygons(gons, [np.asarray(polys[i]["v"])[:int(polys[i]["count"])] for i in gons])
    got = w.bodies
    for field in ("pos", "xv", "yv", "geom_size"):
        assert got[field].tobytes() == bodies[field].tobytes(), "the world's %s are not the corpus's" % field
    return w


def world_polys(w):
    """The world's polygons as the specification takes them: a list of phx_polygon records, one per body."""
    return list(w.polygons())


class Case:
    def __init__(self, name, rows, polys):
        self.name, self.rows, self.polys = name, rows, polys
        self.bodies, self.kinds = records(rows)
        self.B = ref.Bodies(self.bodies, self.kinds, polys)
        self.queries, self.near_queries = [], []

    def add(self, p, max_dist, doubtful=False):
        """The query {p, max_dist} into `queries` if the judge has it clear by DESIGN u, into `near_queries` otherwise."""
        q = np.array([p[0], p[1], max_dist], dtype=F)
        (self.near_queries if doubtful or margin(self.B, q) < DESIGN else self.queries).append(q)

    def done(self):
        self.queries = np.array(self.queries, dtype=F).reshape(-1, 3)
        self.near_queries = np.array(self.near_queries, dtype=F).reshape(-1, 3)
        return self


def margin(B, q):
    """How far the query's answer is from changing, in u, by the judge alone: the smallest of every contender's distance from
    max_dist, the runner-up's lead over the winner and the winner's medial distance."""
    v = ref.near(B, q)
    u = ref.unit(B, q, v)
    r = float(F(q[2]))
    within = v.sd <= r
    if not within.any():
        return float(((v.sd - r) / u).min())
    want = int(np.argmin(np.where(within, v.sd, np.inf)))
    lead = (v.sd - v.sd[want]) / np.maximum(u, u[want])
    lead[want] = np.inf
    contender = lead < DESIGN
    contender[want] = True
    edge = (np.abs(v.sd - r) / u)[contender].min()
    return float(min(edge, lead.min(), v.medial[want] / u[want]))


# ---- the placements ---------------------------------------------------------------------------------------------------------------------
def features(B, b):
    """Body b's surface points with their outward directions, in the world, float64: [(point, direction, "face" | "corner")], the
    faces first."""
    pos, xv, yv, h = B.pos[b], B.xv[b], B.yv[b], B.h[b]
    at = lambda x, y: pos + x * xv + y * yv                                   # noqa: E731
    to = lambda x, y: (x * xv + y * yv) / np.hypot(*(x * xv + y * yv))        # noqa: E731
    kind = int(B.kind[b])
    if kind == CIRCLE:
        return [(pos + h[0] * np.array(d), np.array(d), "face") for d in ((1.0, 0.0), (0.6, 0.8), (-0.28, -0.96), (0.0, -1.0))]
    if kind == CAPSULE:
        r, a = h[1], h[0] - h[1]
        out = [(at(0.3 * a, r), to(0, 1), "face"), (at(-0.7 * a, -r), to(0, -1), "face"), (at(a + r, 0), to(1, 0), "face"), (at(-a - r, 0), to(-1, 0), "face")]
        return out + [(at(a + 0.6 * r, 0.8 * r), to(0.6, 0.8), "corner"), (at(-a - 0.8 * r, -0.6 * r), to(-0.8, -0.6), "corner")]
    if kind == POLYGON:
        v = B.verts[b]
        n = len(v)
        out, normals = [], []
        for k in range(n):
            e = v[(k + 1) % n] - v[k]
            normals.append(np.array([e[1], -e[0]]) / np.hypot(*e))
            s = v[k] + 0.37 * e
            out.append((at(*s), to(*normals[-1]), "face"))
        for k in range(n):
            d = normals[k] + normals[k - 1]
            out.append((at(*v[k]), to(*d), "corner"))
        return out
    faces = [(at(h[0], 0.3 * h[1]), to(1, 0), "face"), (at(-h[0], -0.3 * h[1]), to(-1, 0), "face"),
             (at(0.3 * h[0], h[1]), to(0, 1), "face"), (at(-0.3 * h[0], -h[1]), to(0, -1), "face")]
    return faces + [(at(sx * h[0], sy * h[1]), to(sx, sy), "corner") for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1))]


def add_placements(case, far=True):
    B = case.B
    n = 0
    for b in range(B.n):
        seen = set()
        for s, d, what in features(B, b):
            outs = OUTS + (DISTANCES if far and what not in seen else ())
            seen.add(what)
            for out in outs:
                n += 1
                case.add(s + out * d, FLT_MAX if n % 3 == 0 else 2.0 * out + 10.0)
            for f in INSIDE:
                case.add(B.pos[b] + f * (s - B.pos[b]), 10.0)
        # the medial points: the centre, and of a capsule two more points of its core
        case.add(B.pos[b], 10.0, doubtful=True)
        if B.kind[b] == CAPSULE:
            a = B.h[b, 0] - B.h[b, 1]
            case.add(B.pos[b] + 0.5 * a * B.xv[b], 10.0, doubtful=True)
            case.add(B.pos[b] - a * B.xv[b], 10.0, doubtful=True)
        if B.kind[b] == BOX:                                                # the diagonal inside a corner: equal depth to two faces
            h = B.h[b]
            case.add(B.pos[b] + (h[0] - 0.25 * h.min()) * B.xv[b] + (h[1] - 0.25 * h.min()) * B.yv[b], 10.0, doubtful=True)
    return case


def add_max_dist(case):
    """For a face and a corner of every body, 0.5 and 3 out: max_dist DESIGN u (and a sixteenth) short of the judge's distance and past
    it (clear by design), and at the float32 distance and one ulp either way (doubtful)."""
    B = case.B
    for b in range(B.n):
        seen = set()
        for s, d, what in features(B, b):
            if what in seen:
                continue
            seen.add(what)
            for out in (0.5, 3.0):
                p = np.asarray(s + out * d, dtype=F)
                v = ref.near(B, p)
                u = ref.unit(B, p, v)
                w = int(np.argmin(v.sd))
                step = 1.0625 * DESIGN * u[w]
                for r in (v.sd[w] - step, v.sd[w] + step):
                    if r >= 0:
                        case.add(p, r)
                t = F(v.sd[w])
                if t > 0:
                    for r in (np.nextafter(t, F(0)), t, np.nextafter(t, F(np.inf))):
                        case.add(p, r, doubtful=True)
    return case


@functools.lru_cache(maxsize=None)
def cases():
    """The corpus, built once per process; the tests leave it unchanged."""
    out = [add_max_dist(add_placements(Case("near the origin", *near_set()))).done()]
    for name, shift in (("bodies at 3000", (3000.0, -3000.0)), ("bodies at 1e5", (1e5, 1e5)), ("bodies at -1e5", (-1e5, 1e5))):
        out.append(add_max_dist(add_placements(Case(name, *near_set(shift)), far=False)).done())
    row = Case("a row, the nearer has the higher index", *row_set())
    for x in (0.0, 14.0, 28.0, 42.0, 56.0, 70.0):
        for y in (4.0, -6.0):
            row.add((x + 0.7, y), 100.0)                                    # beside each body in turn: body 0 (x = 42) is in reach of them all
            row.add((x - 1.1, y), FLT_MAX)
    row.add((21.0, 40.0), 100.0)
    B = row.B                                                               # equal distance from the two circles (bodies 0 and 4): doubtful
    mid = 0.5 * (B.pos[0] + B.pos[4]) + 0.5 * (B.h[0, 0] - B.h[4, 0]) * (B.pos[0] - B.pos[4]) / np.hypot(*(B.pos[0] - B.pos[4]))
    row.add(mid, 100.0, doubtful=True)
    out.append(row.done())
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def assert_bounds(worst, what):
    for (kind, m), (figure, q) in worst.items():
        bound = BOUNDS.get((kind, m), BOUND)
        assert figure <= bound, "%s: %s %s is %.3g u at query %d, the bound is %g u" % (what, kind, m, figure, q, bound)


def table(worst):
    return "  ".join("%s %s" % (kind, " ".join("%s %.3g" % (m, worst[(kind, m)][0]) for m in ref.MEASURES)) for kind in ref.KINDS)


# ---- an answer held to the judge --------------------------------------------------------------------------------------------------------
def judge_near(bodies, kinds, polys, queries, got):
    """query_nearest's answer `got` (near_hit_dtype) for `queries` against the judge.  The contenders of a query are the bodies within
    max_dist or within NEAR u of it; the possible winners are the contenders within NEAR u of the nearest of them.  One possible
    winner that is clear of max_dist: the answer must name it.  Otherwise the query is doubtful: the answer names a possible winner,
    or nobody when no body is clearly within max_dist.  Whatever body is named, `distance` is measured against that body's own signed
    distance; `point`, `normal` and `length` too unless the point is within NEAR u of where they jump (near_reference medial; outside
    a corner or a vertex: of its tip).
    Returns (doubtful pairs (K, N) bool, worst {(kind, measure): (figure in u, query index)})."""
    B = ref.Bodies(bodies, kinds, polys)
    pairs = np.zeros((len(queries), B.n), dtype=bool)
    worst = {(k, m): (0.0, -1) for k in ref.KINDS for m in ref.MEASURES}
    for q, row in enumerate(queries):
        v = ref.near(B, row)
        u = ref.unit(B, row, v)
        r = float(F(row[2]))
        b = int(got["body"][q])
        within = v.sd <= r
        edge = np.abs(v.sd - r) <= NEAR * u
        contender = within | edge
        if not contender.any():
            assert b == -1, "query %d %s: body %d, the judge has none within max_dist" % (q, row, b)
            continue
        poss = contender & (v.sd <= v.sd[contender].min() + NEAR * u)
        if poss.sum() == 1 and not edge[poss].any():
            want = int(np.flatnonzero(poss)[0])
            assert b == want, "query %d %s: body %d, the judge has %d" % (q, row, b, want)
        else:
            pairs[q] = poss
            assert (b >= 0 and poss[b]) or (b == -1 and not (within & ~edge).any()), \
                "query %d %s: body %d, the judge's possible winners are %s" % (q, row, b, np.flatnonzero(poss))
        if b < 0:
            continue
        jumpy = bool(v.medial[b] <= NEAR * u[b])
        pairs[q, b] = pairs[q, b] or jumpy
        dev = ref.deviation(B, row, v, b, got[q])
        for m in ref.MEASURES:
            if jumpy and m != "distance":
                continue
            key = (ref.KINDS[int(B.kind[b])], m)
            if dev[m] / u[b] > worst[key][0]:
                worst[key] = (dev[m] / u[b], q)
    return pairs, worst
