"""The float64 judge of tests/capsule_spec.py.  It shares no code with the specification: a capsule here is its core segment with a
radius, a box its four edges, and everything is a distance between segments and points computed in float64 from the same float32
records.  It never forms a candidate and never looks at the spec's intermediate values.

For a pair the judge gives the distance between the two cores (a capsule's segment, a circle's centre, a box's filled rectangle), the
signed depth r1 + r2 - distance (a box has r = 0), and the unit normal from body 2 towards body 1: the direction between the cores'
closest points.  Where the cores themselves meet (distance 0: an end inside the box, crossed segments, a skewered box) there is no
normal and no depth to hold a point to, and the judge claims only that the points lie on the surfaces: `depth` and `normal` are None.

deviation() measures a float32 contact {p1, p2, n} in circle_reference's four measures (length, normal, depth, surface; a measure the
judge has no value for is 0); second() measures a second point: length, surface, and `across`, the component of p2 - p1 across n over
the scale (a contact's two points face each other along its normal), and `disc`: as surface, but a capsule's point may lie on an end
disc's circle instead.  The difference between the two is the rule's, not rounding: a second point that comes from an end disc lies on
that disc's circle along the contact normal, and where the normal leans by theta from the side's own normal that point is
r * (1 - cos(theta)) inside the capsule's side.  It vanishes for a capsule at rest on a face; the corpus leans by 0.05 rad (2.5e-3
for r = 2).

entry() is the judge of the ray and the moving disc: the first t in [0, max_t] at which the signed distance of o + t*d from the
capsule grown by the query's radius is <= 0, found by minimising that convex function along the ray and bisecting in front of the
minimum; with it the clearance (the smallest signed distance over the interval: how far the verdict is from changing)."""
import numpy as np

BOX, CIRCLE, CAPSULE = 0, 1, 2


class Body:
    def __init__(self, rec, kind):
        f = np.float64
        self.pos = np.array([f(rec["pos"]["x"]), f(rec["pos"]["y"])])
        self.xv = np.array([f(rec["xv"]["x"]), f(rec["xv"]["y"])])
        self.yv = np.array([f(rec["yv"]["x"]), f(rec["yv"]["y"])])
        self.h = np.array([f(rec["geom_size"]["x"]), f(rec["geom_size"]["y"])])
        self.kind = int(kind)

    @property
    def radius(self):
        return {BOX: 0.0, CIRCLE: self.h[0], CAPSULE: self.h[1]}[self.kind]

    def core(self):
        """The core as a list of segments (a, b) and whether it has an inside (a box)."""
        if self.kind == CIRCLE:
            return [(self.pos, self.pos)]
        if self.kind == CAPSULE:
            a = np.float64(np.float32(self.h[0]) - np.float32(self.h[1]))      # the one float32 subtraction that defines the capsule
            return [(self.pos - self.xv * a, self.pos + self.xv * a)]
        c = [self.pos + self.xv * sx * self.h[0] + self.yv * sy * self.h[1] for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        return [(c[k], c[(k + 1) % 4]) for k in range(4)]

    def contains(self, p):
        """A box's filled core holds p (closed)."""
        if self.kind != BOX:
            return False
        m = np.array([[self.xv[0], self.yv[0]], [self.xv[1], self.yv[1]]])
        q = np.linalg.solve(m, np.asarray(p, dtype=np.float64) - self.pos)
        return bool((np.abs(q) <= self.h).all())

    def core_distance(self, p):
        p = np.asarray(p, dtype=np.float64)
        if self.contains(p):
            return 0.0
        return min(float(np.hypot(*(p - closest_on_segment(p, a, b)))) for a, b in self.core())

    def surface_distance(self, p):
        """|distance| of the world point p from the body's surface."""
        if self.kind == BOX:
            m = np.array([[self.xv[0], self.yv[0]], [self.xv[1], self.yv[1]]])
            d = np.abs(np.linalg.solve(m, np.asarray(p, dtype=np.float64) - self.pos)) - self.h
            return float(-d.max()) if (d <= 0).all() else float(np.hypot(*np.maximum(d, 0.0)))
        return abs(self.core_distance(p) - self.radius)

    def candidate_distance(self, p):
        """|distance| of p from what a candidate's point lies on: the surface, or, of a capsule, the circle of an end disc (where the
        cores meet, or the contact normal leans from the side's, an end disc's point lies inside the capsule, on that circle)."""
        d = self.surface_distance(p)
        if self.kind == CAPSULE:
            a, b = self.core()[0]
            d = min([d] + [abs(float(np.hypot(*(np.asarray(p, dtype=np.float64) - e))) - self.radius) for e in (a, b)])
        return d


def closest_on_segment(p, a, b):
    ab = b - a
    l2 = float(ab @ ab)
    if l2 == 0.0:
        return a
    return a + ab * min(1.0, max(0.0, float((p - a) @ ab) / l2))


def _cross(u, v):
    return u[0] * v[1] - u[1] * v[0]


def segments_cross(a, b, c, d):
    """The closed segments ab and cd share a point (proper crossings and touching ends; collinear overlaps by their ends)."""
    if np.array_equal(a, b) or np.array_equal(c, d):
        return False
    d1, d2 = _cross(d - c, a - c), _cross(d - c, b - c)
    d3, d4 = _cross(b - a, c - a), _cross(b - a, d - a)
    return bool(d1 * d2 < 0 and d3 * d4 < 0)


def segment_pair(a, b, c, d):
    """(distance, point on ab, point on cd) of two segments that do not cross: the closest pair has an end of one of them."""
    best = None
    for p, s0, s1, flip in ((a, c, d, False), (b, c, d, False), (c, a, b, True), (d, a, b, True)):
        q = closest_on_segment(p, s0, s1)
        dist = float(np.hypot(*(p - q)))
        if best is None or dist < best[0]:
            best = (dist, q, p) if flip else (dist, p, q)
    return best


def cores(b1, b2):
    """(distance, point on core 1, point on core 2); distance 0.0 with no points where the cores meet."""
    best = None
    for a, b in b1.core():
        for c, d in b2.core():
            if segments_cross(a, b, c, d):
                return 0.0, None, None
            got = segment_pair(a, b, c, d)
            if best is None or got[0] < best[0]:
                best = got
    for inner, outer in ((b1, b2), (b2, b1)):
        if outer.kind == BOX and any(outer.contains(p) for seg in inner.core() for p in seg):
            return 0.0, None, None
    if best[0] == 0.0:
        return 0.0, None, None
    return best


def scale(b1, b2):
    return float(max(1.0, np.abs(b1.pos).max(), np.abs(b2.pos).max(), b1.h.max(), b2.h.max()))


def judge(rec1, kind1, rec2, kind2):
    """{"depth": r1 + r2 - the cores' distance, or None where the cores meet; "normal": from body 2 towards body 1, or None;
    "distance"; "bodies"}"""
    b1, b2 = Body(rec1, kind1), Body(rec2, kind2)
    dist, p1, p2 = cores(b1, b2)
    if p1 is None:
        return {"depth": None, "normal": None, "distance": 0.0, "bodies": (b1, b2)}
    return {"depth": float(b1.radius + b2.radius - dist), "normal": (p1 - p2) / dist, "distance": dist, "bodies": (b1, b2)}


def deviation(verdict, p1, p2, n):
    b1, b2 = verdict["bodies"]
    p1, p2, n = (np.asarray(v, dtype=np.float64) for v in (p1, p2, n))
    s = scale(b1, b2)
    length = abs(float(np.hypot(*n)) - 1.0)
    angle, depth = 0.0, 0.0
    if verdict["normal"] is not None:
        u = n / np.hypot(*n)
        angle = abs(float(np.arctan2(_cross(u, verdict["normal"]), u @ verdict["normal"])))
        depth = abs(float((p2 - p1) @ n) - verdict["depth"]) / s
    if verdict["normal"] is None:                                           # the cores meet: the points lie on the surfaces or on an end disc's circle
        surface = max(b1.candidate_distance(p1), b2.candidate_distance(p2)) / s
    else:
        surface = max(b1.surface_distance(p1), b2.surface_distance(p2)) / s
    return {"length": length, "normal": angle, "depth": depth, "surface": surface}


def second(verdict, p1, p2, n):
    b1, b2 = verdict["bodies"]
    p1, p2, n = (np.asarray(v, dtype=np.float64) for v in (p1, p2, n))
    s = scale(b1, b2)
    u = n / np.hypot(*n)
    return {"length": abs(float(np.hypot(*n)) - 1.0), "surface": max(b1.surface_distance(p1), b2.surface_distance(p2)) / s,
            "disc": max(b1.candidate_distance(p1), b2.candidate_distance(p2)) / s, "across": abs(float(_cross(p2 - p1, u))) / s}


# ---- the queries ----------------------------------------------------------------------------------------------------------------------------
def signed_distance(body, p, grow=0.0):
    """The signed distance of p from the capsule grown by `grow` (< 0 inside)."""
    return body.core_distance(p) - (body.radius + grow)


def entry(body, o, d, max_t, grow=0.0):
    """(t or None, clearance): the first t in [0, max_t] with signed_distance <= 0, and how far the verdict is from changing: the
    function's smallest value over the interval (<= 0: a hit, by that margin; > 0: a miss, by that gap)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    f = lambda t: signed_distance(body, o + t * d, grow)      # noqa: E731  (convex in t: the distance from a convex set along a line)
    if f(0.0) <= 0.0:
        return 0.0, f(0.0)
    lo, hi = 0.0, float(max_t)
    for _ in range(100):
        m1, m2 = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
        if f(m1) <= f(m2):
            hi = m2
        else:
            lo = m1
    tm = 0.5 * (lo + hi)
    best = min(f(tm), f(float(max_t)))
    if f(float(max_t)) < f(tm):
        tm = float(max_t)
    if best > 0.0:
        return None, best
    lo, hi = 0.0, tm
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        if f(mid) <= 0.0:
            hi = mid
        else:
            lo = mid
    return hi, best
