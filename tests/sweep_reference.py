"""The float64 judge of tests/sweep_spec.py.  It shares no code and no method with the specification: it never widens a shape, never
splits one into parts and never intersects a ray with anything.  All it knows is the signed distance sd(p) of a point from a target's
outline, in float64 from the same float32 records and vertices:
  a box, a polygon    the outline's world vertices; inside, the largest edge distance; outside, the distance to the nearest edge segment
  a circle, a capsule the distance from the core (a point, a segment) less the radius
and f(t) = sd(s + t*d) - rc, which is convex in t (the distance from a convex set along a line):
  f(0) <= 0           the core overlaps the target at the start: the discrete contact owns the pair, no hit
  otherwise           the minimum of f over [0, 1] is bracketed by ternary search; a minimum > 0 is a miss; otherwise the first t with
                      f(t) <= 0 is found by bisection between 0 and the minimiser, and the normal is the direction from the outline's
                      closest point to the centre there.
The clearance says how far the verdict is from changing: f(0) and -min f for a hit (a start that nearly overlaps, a cast that nearly
misses: a grazing one), min f for a miss, -f(0) for an overlap.  unit() is u = 2^-24 * scale, what a float32 of the sizes involved
can carry; deviation() measures a float32 answer {t, normal} in lengths, as tests/round_query_reference.py does: |t - t_judge| * |d|,
the normal's angle as a length on the radius of curvature rho of the surface the centre meets (rc around a vertex, a circle's r + rc, a
capsule's r + rc at an end; the target's size + rc on a face), and | |normal| - 1 | * rho."""
import numpy as np

from round_query_reference import NEAR      # noqa: F401  (a verdict this many u from changing may be excused)

BOX, CIRCLE, CAPSULE, POLYGON = 0, 1, 2, 3
f8 = np.float64


def _vec(rec, name):
    return np.array([f8(rec[name]["x"]), f8(rec[name]["y"])])


class Target:
    def __init__(self, rec, kind, poly=None):
        self.pos, self.xv, self.yv, self.h = _vec(rec, "pos"), _vec(rec, "xv"), _vec(rec, "yv"), _vec(rec, "geom_size")
        self.kind = int(kind)
        self.outline, self.core, self.radius = None, None, 0.0
        if self.kind == POLYGON:
            self.outline = [self.pos + self.xv * f8(x) + self.yv * f8(y) for x, y in np.asarray(poly["v"])[:int(poly["count"])]]
            self.size = float(self.h.max())
        elif self.kind == BOX:
            self.outline = [self.pos + self.xv * (sx * self.h[0]) + self.yv * (sy * self.h[1]) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
            self.size = float(self.h.max())
        elif self.kind == CIRCLE:
            self.core, self.radius, self.size = (self.pos, self.pos), float(self.h[0]), float(self.h[0])
        else:
            a = f8(np.float32(self.h[0]) - np.float32(self.h[1]))           # the one float32 subtraction that defines the capsule
            self.core, self.radius, self.size = (self.pos - self.xv * a, self.pos + self.xv * a), float(self.h[1]), float(self.h[0])

    def foot(self, p):
        """(the outline's closest point to p, whether p is inside, whether the closest point is a vertex or an end)."""
        if self.outline is None:
            q, end = _on_segment(p, *self.core)
            w = p - q
            l = float(np.hypot(*w))
            return (q + w * (self.radius / l) if l > 0 else q), l <= self.radius, end or self.kind == CIRCLE
        m = len(self.outline)
        best, inside = None, True
        for k in range(m):
            a, b = self.outline[k], self.outline[(k + 1) % m]
            e = b - a
            if (e[1] * (p - a)[0] - e[0] * (p - a)[1]) / np.hypot(*e) > 0:
                inside = False
            q, end = _on_segment(p, a, b)
            dist = float(np.hypot(*(p - q)))
            if best is None or dist < best[0]:
                best = (dist, q, end)
        return best[1], inside, best[2]

    def sd(self, p):
        q, inside, _ = self.foot(p)
        dist = float(np.hypot(*(p - q)))
        return -dist if inside else dist


def _on_segment(p, a, b):
    ab = b - a
    l2 = float(ab @ ab)
    if l2 == 0.0:
        return a, True
    x = float((p - a) @ ab) / l2
    return a + ab * min(1.0, max(0.0, x)), not 0.0 < x < 1.0


class Verdict:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def cast(target, s, rc, d):
    """The core disc {s, rc} along d over t in [0, 1] against one target (float32 values): Verdict(kind, t, normal, clearance, vertex),
    kind "overlap", "miss" or "hit"."""
    s, d, rc = np.asarray(s, dtype=np.float32).astype(f8), np.asarray(d, dtype=np.float32).astype(f8), f8(np.float32(rc))
    f = lambda t: target.sd(s + t * d) - rc      # noqa: E731
    f0 = f(0.0)
    if f0 <= 0.0:
        return Verdict(kind="overlap", t=None, normal=None, clearance=-f0, vertex=False)
    lo, hi = 0.0, 1.0
    for _ in range(120):
        m1, m2 = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
        if f(m1) <= f(m2):
            hi = m2
        else:
            lo = m1
    tm = 0.5 * (lo + hi)
    if f(1.0) < f(tm):
        tm = 1.0
    fm = f(tm)
    if fm > 0.0:
        return Verdict(kind="miss", t=None, normal=None, clearance=fm, vertex=False)
    lo, hi = 0.0, tm
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if f(mid) <= 0.0:
            hi = mid
        else:
            lo = mid
    at = s + hi * d
    q, _, vertex = target.foot(at)
    n = at - q
    n = n / np.hypot(*n)
    # (a cast that ends on the outline at exactly t = 1 has -fm = 0: it is as close to missing as a grazing one)
    return Verdict(kind="hit", t=hi, normal=n, clearance=min(f0, -fm), vertex=vertex)


def unit(target, s, rc, d, t=0.0):
    s, d = np.asarray(s, dtype=f8), np.asarray(d, dtype=f8)
    return 2.0 ** -24 * max(1.0, float(np.hypot(*s)), float(np.hypot(*target.pos)), target.size, float(rc), float(t) * float(np.hypot(*d)))


def rho(target, rc, v):
    if target.kind == CIRCLE:
        return target.radius + float(rc)
    if target.kind == CAPSULE:
        return (target.radius if v.vertex else target.size) + float(rc)
    return float(rc) if v.vertex else target.size + float(rc)


def deviation(target, rc, d, v, t, normal):
    """The measures of a float32 answer {t, normal} for a cast the judge's Verdict v calls a hit, in lengths."""
    d = np.asarray(d, dtype=np.float32).astype(f8)
    n = np.asarray(normal, dtype=f8)
    size = rho(target, rc, v)
    return {"hit": abs(f8(t) - v.t) * float(np.hypot(*d)),
            "normal": abs(float(np.arctan2(n[0] * v.normal[1] - n[1] * v.normal[0], n @ v.normal))) * size,
            "length": abs(float(np.hypot(*n)) - 1.0) * size}
