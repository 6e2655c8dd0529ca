"""A directed corpus for the point and ray queries at the scale of the project's worlds (tests/query_reference.py is its judge): small
sets of discs and boxes, and rays and points placed against each of them by construction.

What varies: the distance of a ray's origin from the body it is aimed at (1 .. 10^6 units, bodies near the world's origin), the
distance of the bodies from the world's origin (3000, 10^5, the ray's origin near them), disc radii 0.5 .. 8 and one of 500, box half
extents 0.5 .. 20 at angles that include 0 and pi / 2 exactly and 1e-3, direction lengths 1e-3, 1 and 1e3, the line through the centre
and at 0.5 and 0.9 of the half width, past the body at 1.5, origins inside, a diagonal across a disc's frame square that misses the
disc, and several discs in a row seen from 3000 units.

A case's `rays` and `points` are the ones whose verdict is clear BY DESIGN: a query is generated only where the designed clearance (the
half width times the distance of the fraction from 1) is at least DESIGN u, u = 2^-24 * the largest coordinate involved, so that the
judge's excused share stays small whatever the code under test does (the tests assert the share against CAP).  `near_rays` and
`near_points` are the deliberately doubtful ones: grazing at 0.999 and 1.001 of the half width, max_t one ulp short of, at and one ulp
beyond the entry.  They are only asserted to be excused or right."""
import functools

import numpy as np

from phyx_amd.api import frame_from_angle, rigid_body_dtype
import query_reference as ref

F = np.float32
BOX, CIRCLE = 0, 1
NEAR = ref.NEAR         # a verdict within this many u of changing may be excused ...
CAP = 0.02              # ... and at most this share of a case's (query, body) pairs
BOUND = 16.0            # every deviation() measure of a hit both sides agree on, in u: a rule is a chain of about a dozen float32
                        # operations on quantities no larger than scale, each contributing at most 1 u
# ... but one: a box's `hit`.  The ray enters through an edge it meets at the angle phi, and the entry t = (lo - o') / d' divides
# what the roundings of o' (the origin in the body's frame, a few u) amount to by d' = |d| sin(phi): along the ray the hit point is
# off by 1 / sin(phi) times the rounding, for any rule that works in float32 coordinates of that size.  The corpus has entries down to
# phi = 13.5 degrees (1 / sin = 4.3); the worst the specification measures is 16.7 u, at phi = 21.9 degrees (1 / sin = 2.7: from 1
# unit, |d| = 1e-3, the long edge of the 20 x 8 box at 0.262 rad).  64 is the smallest power of two that holds with a factor 2 to
# spare.  A disc has no such term: its `hit` stays at BOUND.
BOUNDS = {("box", "hit"): 64.0}
DESIGN = 64.0           # the designed clearance of a query in `rays` / `points`, in u: twice NEAR
DISTANCES = (1.0, 30.0, 300.0, 3000.0, 30000.0, 1e6)
LENGTHS = (1.0, 1e-3, 1e3)
EXACT = {"0": (1.0, 0.0, 0.0, 1.0), "pi/2": (0.0, 1.0, -1.0, 0.0)}      # frames no angle's cos / sin gives exactly


def records(rows):
    """Bodies (px, py, angle, hx, hy, kind) as add_body frames them (angle "0" or "pi/2": the exact frame, as set_poses can store it);
    the AABB is pos -/+ (|xv|*h.x + |yv|*h.y) in float32, as UpdateGeom computes it.  Returns (records, kinds)."""
    b = np.zeros(len(rows), dtype=rigid_body_dtype)
    for i, (px, py, ang, hx, hy, _) in enumerate(rows):
        fr = np.array([px, py, *EXACT[ang]], dtype=F) if isinstance(ang, str) else frame_from_angle(px, py, ang)
        b[i]["index"] = i
        b[i]["pos"] = b[i]["geom_pos"] = tuple(fr[0:2])
        b[i]["xv"] = b[i]["geom_xv"] = tuple(fr[2:4])
        b[i]["yv"] = b[i]["geom_yv"] = tuple(fr[4:6])
        b[i]["geom_size"] = (hx, hy)
        ex = np.abs(fr[2]) * F(hx) + np.abs(fr[4]) * F(hy)
        ey = np.abs(fr[3]) * F(hx) + np.abs(fr[5]) * F(hy)
        b[i]["aabb_min"] = (fr[0] - ex, fr[1] - ey)
        b[i]["aabb_max"] = (fr[0] + ex, fr[1] + ey)
        b[i]["inv_mass"], b[i]["inv_inertia"] = 1, 1
    return b, np.array([r[5] for r in rows], dtype=np.int32)


def frames(bodies):
    """The (N, 6) poses of World.set_poses that store the records' frames exactly."""
    return np.stack([bodies["pos"]["x"], bodies["pos"]["y"], bodies["xv"]["x"], bodies["xv"]["y"], bodies["yv"]["x"], bodies["yv"]["y"]], axis=1).astype(F)


def world(bodies, kinds):
    """A device world that holds the records' bodies: add_bodies, set_poses with the exact frames, set_shapes for the discs; no step."""
    import phyx_amd
    w = phyx_amd.World(0, gravity=0.0)
    n = len(bodies)
    rows = np.stack([bodies["pos"]["x"], bodies["pos"]["y"], np.zeros(n), bodies["geom_size"]["x"], bodies["geom_size"]["y"]], axis=1).astype(F)
    idx = w.add_bodies(rows)
    w.set_poses(idx, frames(bodies))
    discs = np.flatnonzero(np.asarray(kinds) == CIRCLE).astype(np.int32)
    if len(discs):
        w.set_shapes(discs, phyx_amd.SHAPE_CIRCLE, bodies["geom_size"]["x"][discs])
    got = w.bodies
    for field in ("pos", "xv", "yv", "geom_size"):
        assert got[field].tobytes() == bodies[field].tobytes(), "the world's %s are not the corpus's" % field
    return w


_judged = {}


def judged(what, judge, bodies, kinds, queries, got):
    """judge(bodies, kinds, queries, got), made once for the same bytes (the two query paths give the same answer: one judgement)."""
    key = (what, bodies.tobytes(), np.asarray(kinds).tobytes(), queries.tobytes(), got.tobytes())
    if key not in _judged:
        _judged[key] = judge(bodies, kinds, queries, got)
    return _judged[key]


class Case:
    def __init__(self, name, rows):
        self.name, self.rows = name, rows
        self.bodies, self.kinds = records(rows)
        self.rays, self.near_rays, self.points, self.near_points = [], [], [], []

    def done(self):
        for k, width in (("rays", 5), ("near_rays", 5), ("points", 2), ("near_points", 2)):
            setattr(self, k, np.array(getattr(self, k), dtype=F).reshape(-1, width))
        return self


# ---- the body sets ----------------------------------------------------------------------------------------------------------------------
def small_set(shift=(0.0, 0.0)):
    """Five discs and ten boxes near a grid 90 apart around `shift`.  The discs' frames are exact, so that a disc's AABB is its frame
    square and a diagonal can cross the square's corner."""
    rows = []
    radii = (0.5, 1.0, 2.0, 4.0, 8.0)
    halves = ((0.5, 0.5), (1.0, 3.0), (5.0, 2.0), (20.0, 8.0), (20.0, 20.0), (0.5, 20.0), (3.0, 3.0), (12.0, 0.5), (7.0, 4.0), (2.0, 1.0))
    angles = ("0", "pi/2", 1e-3, 0.262, 4.189, "0", -1e-3, "pi/2", 2.827, 5.0)
    spots = [(x, y) for y in (-90.0, 0.0, 90.0) for x in (-180.0, -90.0, 0.0, 90.0, 180.0)]
    order = [0, 5, 1, 6, 2, 7, 3, 8, 4, 9, 10, 11, 12, 13, 14]           # discs and boxes alternate
    discs, boxes = iter(radii), iter(zip(halves, angles))
    for i, (k, (x, y)) in enumerate(zip(order, spots)):
        x, y = x + 1.7 * ((i * 7) % 5), y + 2.3 * ((i * 3) % 7)           # (off the grid: no ray at one body is tangent to another)
        if k < 5:
            r = next(discs)
            rows.append((x + shift[0], y + shift[1], "0", r, r, CIRCLE))
        else:
            (hx, hy), a = next(boxes)
            rows.append((x + shift[0], y + shift[1], a, hx, hy, BOX))
    return rows


def big_set():
    """The disc of radius 500 with a small disc and a box beside it."""
    return [(0.0, 0.0, "0", 500.0, 500.0, CIRCLE), (900.0, 0.0, "0", 2.0, 2.0, CIRCLE), (0.0, 900.0, 0.262, 5.0, 2.0, BOX)]


def row_set(y=0.0):
    """Discs in a row along x, 6 apart, the index order scrambled: seen along the row, the nearest is never body 0."""
    xs = (18.0, 6.0, 30.0, 0.0, 12.0, 24.0)
    return [(x, y, "0", 1.0 + 0.25 * (i % 3), 1.0 + 0.25 * (i % 3), CIRCLE) for i, x in enumerate(xs)]


# ---- the queries ------------------------------------------------------------------------------------------------------------------------
DIRECTIONS = (0.0, np.pi / 2, float(np.arctan2(0.6, 0.8)), 7.0 * np.pi / 6.0, -np.pi / 4)


def _geometry(row, e):
    """(centre, half width across e, reach along e) of a body row for the unit direction e, in float64 from the stored floats."""
    b, k = records([row])
    B = ref.Bodies(b, k)
    if k[0] == CIRCLE:
        return B.pos[0], B.r[0], B.r[0]
    p = np.array([-e[1], e[0]])
    across = abs(B.xv[0] @ p) * B.h[0, 0] + abs(B.yv[0] @ p) * B.h[0, 1]
    along = abs(B.xv[0] @ e) * B.h[0, 0] + abs(B.yv[0] @ e) * B.h[0, 1]
    return B.pos[0], across, along


def _u(*lengths):
    return 2.0 ** -24 * max(1.0, *lengths)


def _aimed(c, w, reach, e, f, dist, length):
    """The ray along e whose line passes the centre c at f * w, starting dist before the body; d = e * length."""
    p = np.array([-e[1], e[0]])
    o = c - (dist + reach) * e + f * w * p
    return [o[0], o[1], e[0] * length, e[1] * length, 2.0 * (dist + 2.0 * reach) / length + 1.0]


def add_rays(case, dist, fractions=(0.0, 0.5, -0.5, 0.9, -0.9, 1.5), graze=(0.999, -0.999, 1.001, -1.001)):
    """Rays at every body of the case from `dist`, in every direction, at every fraction that is clear by design; the grazing ones and
    the max_t ones go to near_rays."""
    n = 0
    for row in case.rows:
        for th in DIRECTIONS:
            e = np.array([np.cos(th), np.sin(th)])
            c, w, reach = _geometry(row, e)
            u = _u(dist + reach + np.hypot(*c), w, reach)
            length = LENGTHS[n % 3]
            n += 1
            for f in fractions:
                if w * abs(1.0 - abs(f)) >= DESIGN * u:
                    case.rays.append(_aimed(c, w, reach, e, f, dist, length))
            for f in graze:
                case.near_rays.append(_aimed(c, w, reach, e, f, dist, length))
            if th == DIRECTIONS[2] and w * 0.5 >= DESIGN * u:           # max_t at the entry, one ulp short of it and one beyond
                r = _aimed(c, w, reach, e, 0.5, dist, length)
                v = ref.ray(ref.Bodies(*records([row])), r)
                t = F(v.t[0])
                case.near_rays += [r[:4] + [m] for m in (np.nextafter(t, F(0)), t, np.nextafter(t, F(np.inf)))]
                short = min(reach, 0.5 * dist)
                if short >= DESIGN * u:
                    case.rays.append(r[:4] + [float(t) - short / length])      # well short of the body: a clear miss
            if row[5] == CIRCLE and th == DIRECTIONS[4] and 0.2 * w >= DESIGN * u:
                case.rays.append(_aimed(c, w, reach, e, 1.2, dist, length))   # across the frame square's corner, past the disc
        c, inner = _geometry(row, np.array([1.0, 0.0]))[0], min(row[3], row[4])
        if 0.5 * inner >= DESIGN * _u(np.hypot(*c), row[3], row[4]):    # the origin inside
            case.rays += [[c[0] + 0.3 * inner, c[1] - 0.2 * inner, 0.6, 0.8, 10.0], [c[0], c[1], -1e-3, 2e-3, 1.0]]
    return case


def add_points(case):
    for row in case.rows:
        b, k = records([row])
        B = ref.Bodies(b, k)
        c, xv, yv, h = B.pos[0], B.xv[0], B.yv[0], B.h[0]
        u = _u(np.hypot(*c), h.max())
        if k[0] == CIRCLE:
            arms = [h[0] * np.array(d) for d in ((1.0, 0.0), (0.6, 0.8), (-0.28, -0.96), (0.0, -1.0))]
        else:
            arms = [h[0] * xv, -h[1] * yv, h[0] * xv + h[1] * yv, -h[0] * xv + h[1] * yv]
        size = h.min()                                                  # (a point at f along an arm is at least |1 - f| * this from the surface)
        for a in arms:
            for f in (0.0, 0.5, 0.9, 1.5):
                if size * abs(1.0 - f) >= DESIGN * u:
                    case.points.append(c + f * a)
            case.near_points += [c + 0.999 * a, c + 1.001 * a]
    return case


@functools.lru_cache(maxsize=None)
def cases():
    """The corpus, built once per process; the tests leave it unchanged."""
    out = []
    for dist in DISTANCES:
        out.append(add_rays(Case("from %g" % dist, small_set()), dist).done())
    out.append(add_rays(add_rays(Case("big disc", big_set()), 30.0), 1e6).done())
    for name, shift in (("bodies at 3000", (3000.0, -3000.0)), ("bodies at -3000", (-3000.0, 3000.0)),
                        ("bodies at 1e5", (1e5, 1e5)), ("bodies at -1e5", (-1e5, 1e5))):
        out.append(add_points(add_rays(Case(name, small_set(shift)), 30.0)).done())
    out.append(add_points(Case("points near the origin", small_set() + big_set()[:1])).done())
    row = Case("a row of discs from 3000", row_set())
    for y in (0.0, 0.5, -0.9, 1.1):                                     # (1.1: past the first discs of radius 1, into a larger one)
        row.rays += [[-3000.0, y, 1.0, 0.0, 4000.0], [3030.0, y, -1e3, 0.0, 4.0], [-3000.0, y, 1.0, 0.0, 2990.0]]
    out.append(row.done())
    many = small_set() + small_set((3000.0, 700.0)) + small_set((-3000.0, 700.0)) + small_set((0.0, 3000.0)) + row_set(-3000.0)[:5]
    assert len(many) == 65
    out.append(add_points(add_rays(Case("65 bodies", many), 300.0, fractions=(0.0, 0.9), graze=())).done())
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def boxes_only(c):
    """The case's boxes alone, as a world without a shape column has them: (records, kinds)."""
    keep = c.kinds == BOX
    return c.bodies[keep], c.kinds[keep]


def assert_bounds(worst, what):
    for (kind, m), (figure, q) in worst.items():
        bound = BOUNDS.get((kind, m), BOUND)
        assert figure <= bound, "%s: %s %s is %.3g u at ray %d, the bound is %g u" % (what, kind, m, figure, q, bound)


def table(worst):
    return "  ".join("%s %s" % (kind, " ".join("%s %.3g" % (m, worst[(kind, m)][0]) for m in ref.MEASURES)) for kind in ("box", "disc"))


# ---- an answer held to the judge --------------------------------------------------------------------------------------------------------
def judge_hits(bodies, kinds, rays, got):
    """raycast's answer `got` (ray_hit_dtype) for `rays` against the judge.  A ray is doubtful when some body's clearance is within
    NEAR u, or two bodies' entries lie within NEAR u of each other at the front.  Every other ray must name the judge's closest body,
    with a normal of (0, 0) exactly when the judge has the origin inside.  Where the named body is one the judge sees hit, the
    deviation() measures are collected whether the ray is doubtful or not (a doubtful verdict does not excuse a poor hit point), except
    `hit` and `surface` of a shallow chord (clearance within NEAR u: its ends move faster than the line).  A doubtful ray is only held
    to naming a body the judge sees hit, or one within NEAR u of it, and to no hit only when every hit the judge sees is that close.
    Returns (doubtful (K,) bool, worst {("box" | "disc", measure): (figure in u, ray index)})."""
    B = ref.Bodies(bodies, kinds)
    doubtful = np.zeros(len(rays), dtype=bool)
    worst = {(k, m): (0.0, -1) for k in ("box", "disc") for m in ref.MEASURES}
    for q, r in enumerate(rays):
        v = ref.ray(B, r)
        u = ref.unit(B, r, v)
        dlen = float(np.hypot(F(r[2]).astype(np.float64), F(r[3]).astype(np.float64)))
        close = v.clearance <= NEAR * u
        want = ref.closest(v)
        front = np.where(v.hit, v.t, np.inf) * dlen
        if want >= 0:
            rivals = (front <= front[want] + NEAR * u) & v.hit
            rivals[want] = False
        doubtful[q] = close.any() or (want >= 0 and rivals.any())
        b = int(got["body"][q])
        if not doubtful[q]:
            assert b == want, "ray %d %s: body %d, the judge has %d" % (q, r, b, want)
        elif b >= 0:
            assert v.hit[b] or close[b], "ray %d %s: body %d, which the judge sees missed by %g u" % (q, r, b, v.clearance[b] / u[b])
        else:
            assert not (v.hit & ~close).any(), "ray %d %s: no hit, the judge has body %d clear by %g u" % (q, r, want, v.clearance[want] / u[want])
        if b < 0 or not v.hit[b]:
            continue
        normal = (float(got["normal"][q][0]), float(got["normal"][q][1]))
        if not close[b] and abs(v.tin[b]) * dlen > NEAR * u[b]:
            assert (normal == (0.0, 0.0)) == bool(v.inside[b]), "ray %d %s: normal %s, inside %s" % (q, r, normal, v.inside[b])
        if normal == (0.0, 0.0):
            v.normal[b] = np.nan
        dev = ref.deviation(B, r, v, b, got["t"][q], normal, got["point"][q])
        for m in ref.MEASURES:
            if close[b] and m in ("hit", "surface"):
                continue
            key = ("disc" if B.round[b] else "box", m)
            if dev[m] / u[b] > worst[key][0]:
                worst[key] = (dev[m] / u[b], q)
    return doubtful, worst


def judge_points(bodies, kinds, points, got, verdicts=None):
    """query_points' answer against the judge: the lowest body whose signed distance is <= 0, unless some body is within NEAR u of
    its surface; then the answer holds the point or nearly, and so does no clear body below it.  verdicts(p) -> (N,) bool, the rule's
    own verdict on every body, equals the judge's on every pair that is not that close.  Returns the doubtful pairs (K, N) bool."""
    B = ref.Bodies(bodies, kinds)
    doubtful = np.zeros(len(points), dtype=bool)
    pairs = np.zeros((len(points), B.n), dtype=bool)
    for q, p in enumerate(points):
        sd = ref.point(B, np.asarray(p, dtype=F).astype(np.float64))
        u = ref.unit(B, p)
        inside = np.flatnonzero(sd <= 0)
        want = int(inside[0]) if len(inside) else -1
        pairs[q] = np.abs(sd) <= NEAR * u
        doubtful[q] = pairs[q].any()
        if verdicts is not None:
            wrong = (np.asarray(verdicts(p), dtype=bool) != (sd <= 0)) & ~pairs[q]
            assert not wrong.any(), "point %d %s: bodies %s, the judge has them at %s u" % (q, p, np.flatnonzero(wrong), (sd / u)[wrong])
        b = int(got[q])
        if not doubtful[q]:
            assert b == want, "point %d %s: body %d, the judge has %d" % (q, p, b, want)
        else:                                                           # the answer holds the point or nearly, and so does no clear body below it
            near = np.abs(sd) <= NEAR * u
            assert (b < 0 or sd[b] <= 0 or near[b]) and not ((sd <= 0) & ~near)[:b if b >= 0 else B.n].any(), \
                "point %d %s: body %d, the judge has %d" % (q, p, b, want)
    return pairs


def judge_pairs(bodies, kinds, rays, verdicts):
    """Every (ray, body) pair: verdicts(r) -> (N,) bool, the rule's own verdict on every body, equals the judge's wherever the clearance
    exceeds NEAR u.  Returns the doubtful pairs (K, N) bool."""
    B = ref.Bodies(bodies, kinds)
    doubtful = np.zeros((len(rays), B.n), dtype=bool)
    for q, r in enumerate(rays):
        v = ref.ray(B, r)
        doubtful[q] = v.clearance <= NEAR * ref.unit(B, r, v)
        wrong = (np.asarray(verdicts(r), dtype=bool) != v.hit) & ~doubtful[q]
        assert not wrong.any(), "ray %d %s: bodies %s, the judge says hit = %s, clear by %s u" % (
            q, r, np.flatnonzero(wrong), v.hit[wrong], (v.clearance / ref.unit(B, r, v))[wrong])
    return doubtful
