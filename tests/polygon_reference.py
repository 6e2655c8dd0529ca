"""The float64 judge of tests/polygon_spec.py.  It shares no code with the specification: every body here is a convex outline in the
world, a list of float64 vertices (a box's four corners, a polygon's own) or a core (a circle's centre, a capsule's segment) with a
radius, all computed in float64 from the same float32 records and vertices.  It never clips, never forms a candidate and never looks at
the spec's intermediate values.

For a pair the judge gives the penetration depth and its axis:
  outline / outline     the separating-axis test over all edge normals of both bodies: the axis of smallest overlap;
  core / outline        the signed distance between the core (a point, a segment) and the outline, less the radius: where the core is
                        outside the outline, the direction between the closest points; where it is inside or crosses it, the
                        separating-axis test over the outline's edge normals and the segment's two normals.
`axes` holds every axis whose overlap is within TIE of the smallest (two faces can be equally shallow, and which the float32 rule
picks is then rounding): a contact's normal is held to the nearest of them.  Normals point from body 2 towards body 1.

deviation() measures a float32 contact {p1, p2, n}: `length` | |n| - 1 |, `normal` the angle from the nearest accepted axis, `surface`
the larger distance of p1 from body 1's surface and p2 from body 2's over the scale, and, for the pair's deepest point only, `depth`:
| (p2 - p1) . n - the judge's depth | over the scale.

inside() and entry() judge the point and the ray: the signed distance of a point from the outline, and the first t in [0, max_t] at
which it is <= 0, by minimising that convex function along the ray and bisecting, with the clearance (how far the verdict is from
changing)."""
import numpy as np

BOX, CIRCLE, CAPSULE, POLYGON = 0, 1, 2, 3
TIE = 1e-5


def _f(x):
    return np.float64(x)


class Body:
    def __init__(self, rec, kind, poly=None):
        self.pos = np.array([_f(rec["pos"]["x"]), _f(rec["pos"]["y"])])
        self.xv = np.array([_f(rec["xv"]["x"]), _f(rec["xv"]["y"])])
        self.yv = np.array([_f(rec["yv"]["x"]), _f(rec["yv"]["y"])])
        self.h = np.array([_f(rec["geom_size"]["x"]), _f(rec["geom_size"]["y"])])
        self.kind = int(kind)
        self.outline, self.core, self.radius = None, None, 0.0
        if self.kind == POLYGON:
            local = np.asarray(poly["v"], dtype=np.float64)[:int(poly["count"])]
            self.outline = [self.pos + self.xv * x + self.yv * y for x, y in local]
        elif self.kind == BOX:
            self.outline = [self.pos + self.xv * sx * self.h[0] + self.yv * sy * self.h[1] for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        elif self.kind == CIRCLE:
            self.core, self.radius = (self.pos, self.pos), float(self.h[0])
        else:
            a = _f(np.float32(self.h[0]) - np.float32(self.h[1]))            # the one float32 subtraction that defines the capsule
            self.core, self.radius = (self.pos - self.xv * a, self.pos + self.xv * a), float(self.h[1])

    def edges(self):
        """(a, b, outward unit normal) of every edge of the outline (counter-clockwise in the body's frame; the frame may be a
        reflection-free rotation only, so the turn is kept in the world)."""
        n = len(self.outline)
        out = []
        for k in range(n):
            a, b = self.outline[k], self.outline[(k + 1) % n]
            e = b - a
            out.append((a, b, np.array([e[1], -e[0]]) / np.hypot(*e)))
        return out

    def signed_distance(self, p):
        """< 0 inside.  An outline: the largest edge distance inside, the distance to the nearest edge segment outside."""
        p = np.asarray(p, dtype=np.float64)
        if self.outline is None:
            return float(np.hypot(*(p - _closest_on_segment(p, *self.core)))) - self.radius
        ds = [float(n @ (p - a)) for a, _, n in self.edges()]
        if max(ds) <= 0.0:
            return max(ds)
        return min(float(np.hypot(*(p - _closest_on_segment(p, a, b)))) for a, b, _ in self.edges())

    def surface_distance(self, p):
        return abs(self.signed_distance(p))


def _closest_on_segment(p, a, b):
    ab = b - a
    l2 = float(ab @ ab)
    if l2 == 0.0:
        return a
    return a + ab * min(1.0, max(0.0, float((p - a) @ ab) / l2))


def _cross(u, v):
    return u[0] * v[1] - u[1] * v[0]


def scale(b1, b2):
    return float(max(1.0, np.abs(b1.pos).max(), np.abs(b2.pos).max(), b1.h.max(), b2.h.max()))


def _support_min(points, n, origin):
    return min(float(n @ (q - origin)) for q in points)


def _outline_outline(A, B):
    """[(separation, axis from B towards A)] over every edge normal of both."""
    out = []
    for a, _, n in A.edges():
        out.append((_support_min(B.outline, n, a), -n))
    for a, _, n in B.edges():
        out.append((_support_min(A.outline, n, a), n))
    return out


def _core_outline(C, P):
    """The core of C (a point or a segment, radius r) against the outline P: [(separation, axis from P towards C)]."""
    a, b = C.core
    ends = [a] if np.array_equal(a, b) else [a, b]
    crossing = any(P.signed_distance(e) <= 0.0 for e in ends)
    if not crossing and len(ends) == 2:                                      # the segment may pass through the outline with both ends outside
        n = len(P.outline)
        for k in range(n):
            c, d = P.outline[k], P.outline[(k + 1) % n]
            if _cross(d - c, a - c) * _cross(d - c, b - c) < 0 and _cross(b - a, c - a) * _cross(b - a, d - a) < 0:
                crossing = True
    if not crossing:                                                         # the closest pair has an end of the core or a vertex of the outline
        best = None
        for e in ends:
            for c, d, _ in P.edges():
                q = _closest_on_segment(e, c, d)
                dist = float(np.hypot(*(e - q)))
                if best is None or dist < best[0]:
                    best = (dist, (e - q) / dist if dist > 0 else None)
        if len(ends) == 2:
            for w in P.outline:
                q = _closest_on_segment(w, a, b)
                dist = float(np.hypot(*(q - w)))
                if dist < best[0]:
                    best = (dist, (q - w) / dist if dist > 0 else None)
        if best[1] is not None:
            return [(best[0] - C.radius, best[1])]
    out = []
    for c, _, n in P.edges():
        out.append((_support_min(ends, n, c) - C.radius, n))
    if len(ends) == 2:
        e = b - a
        m = np.array([e[1], -e[0]]) / np.hypot(*e)
        for s in (m, -m):
            out.append((_support_min(P.outline, s, a) - C.radius, -s))
    return out


def judge(rec1, kind1, poly1, rec2, kind2, poly2):
    """{"depth", "axes": the accepted unit normals from body 2 towards body 1, "bodies"}"""
    b1, b2 = Body(rec1, kind1, poly1), Body(rec2, kind2, poly2)
    if b1.outline is not None and b2.outline is not None:
        found = _outline_outline(b1, b2)
    elif b1.outline is None:
        found = _core_outline(b1, b2)
    else:
        found = [(s, -n) for s, n in _core_outline(b2, b1)]
    sep = max(s for s, _ in found)
    return {"depth": -sep, "axes": [n for s, n in found if s >= sep - TIE], "bodies": (b1, b2)}


def deviation(verdict, p1, p2, n, deepest=True):
    b1, b2 = verdict["bodies"]
    p1, p2, n = (np.asarray(v, dtype=np.float64) for v in (p1, p2, n))
    s = scale(b1, b2)
    u = n / np.hypot(*n)
    angle = min(abs(float(np.arctan2(_cross(u, a), u @ a))) for a in verdict["axes"])
    return {"length": abs(float(np.hypot(*n)) - 1.0), "normal": angle,
            "depth": abs(float((p2 - p1) @ n) - verdict["depth"]) / s if deepest else 0.0,
            "surface": max(b1.surface_distance(p1), b2.surface_distance(p2)) / s}


# ---- the queries ----------------------------------------------------------------------------------------------------------------------------
def inside(body, p):
    """(inside (closed), the signed distance: how far the verdict is from changing)"""
    d = body.signed_distance(p)
    return d <= 0.0, d


def entry(body, o, d, max_t):
    """(t or None, clearance): the first t in [0, max_t] with signed_distance <= 0, and the function's smallest value over the interval."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    f = lambda t: body.signed_distance(o + t * d)      # noqa: E731  (convex in t outside the body; one minimum along a line)
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


def edge_normal(body, p):
    """The outward normal of the outline's edge nearest the world point p."""
    p = np.asarray(p, dtype=np.float64)
    return min(body.edges(), key=lambda e: float(np.hypot(*(p - _closest_on_segment(p, e[0], e[1])))))[2]
