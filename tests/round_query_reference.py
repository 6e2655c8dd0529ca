"""The float64 judge of the round queries (include/phyx_amd.h, QUERIES: query circles and circle casts): what a circle overlaps and
what a moving circle touches first, computed in float64 from the same float32 records and kinds, and the measures a float32 answer is
held to.  It shares no code and no method with tests/round_query_spec.py: it never widens a box, splits it into parts or intersects a
ray with anything.  All it knows is the signed distance sd(p) of a point from a body (a box's in its frame, the point's coordinates
found by solving against the float32 frame, not by projecting on it, as circle_reference.Body.local; a disc's |p - pos| - rb):
  overlap   the circle {c, r} overlaps a body iff sd(c) <= r; the clearance is |sd(c) - r|;
  cast      f(t) = sd(c + t*d) - r is convex in t (the distance from a convex set along a line).  f(0) <= 0: the cast starts
            overlapping, t = 0.  Otherwise f is minimised over [0, max_t] by golden section; a minimum > 0 is a miss with that minimum
            as its clearance; otherwise the first root is found by bisection between 0 and the minimiser, and the normal is the
            direction from the body's closest point to the centre there.  A hit's clearance is the smaller of f(0) (how far the start
            is from overlapping: there t and the normal change their kind) and -min f (how far the cast is from missing).

Everything is vectorised over the bodies: one query against all of them.
  Bodies                       the float64 columns of the records
  sd(B, p)                     the signed distance of p (2,) or (N, 2) from every body
  overlap(B, c)                (hit, clearance) per body
  cast(B, c)                   Verdict per body: hit, t, inside, normal, clearance (and what rho() needs)
  closest(v)                   the closest hit of a Verdict (smallest t, then the lowest index), -1 if none
  unit(B, q, v)                u = 2^-24 * scale per body, scale = the largest of 1, |c|, |pos|, the sizes, r and t*|d|
  deviation(B, c, v, b, t, normal)    the measures of a float32 answer {t, normal} for body b, in lengths

rho is the radius of curvature of the surface the centre meets (the body widened by r) at the judge's hit: r + rb on a circle body, r
around a box's corner, and for a face, which has none, the box's larger half extent + r.  A normal's error is measured as a length on
that radius, as query_reference.deviation measures a ray's on the body's size: around a corner the normal of a small circle turns by
1 / r per unit of length, for any rule."""
import numpy as np

BOX, CIRCLE = 0, 1
f8 = np.float64
NEAR = 32.0             # a verdict this many u from changing may be excused (query_reference.NEAR)
MEASURES = ("hit", "normal", "length")
GOLD = (np.sqrt(5.0) - 1.0) / 2.0


class Bodies:
    def __init__(self, records, kinds):
        b = np.asarray(records)
        col = lambda name: np.stack([b[name]["x"].astype(f8), b[name]["y"].astype(f8)], axis=1)      # noqa: E731
        self.n = len(b)
        self.pos, self.xv, self.yv, self.h = col("pos"), col("xv"), col("yv"), col("geom_size")
        self.round = np.zeros(self.n, dtype=bool) if kinds is None else np.asarray(kinds).astype(np.int64) == CIRCLE
        self.rb = self.h[:, 0]
        self.size = np.where(self.round, self.rb, self.h.max(axis=1))
        self.det = self.xv[:, 0] * self.yv[:, 1] - self.xv[:, 1] * self.yv[:, 0]

    def local(self, p):
        """p (2,) or (N, 2) in every body's frame: the solution of pos + a*xv + b*yv = p."""
        q = np.asarray(p, dtype=f8) - self.pos
        a = (q[:, 0] * self.yv[:, 1] - q[:, 1] * self.yv[:, 0]) / self.det
        b = (self.xv[:, 0] * q[:, 1] - self.xv[:, 1] * q[:, 0]) / self.det
        return np.stack([a, b], axis=1)


def sd(B, p):
    """< 0 inside, > 0 outside.  (A frame's axes have length 1 to float32 accuracy, so a box's local coordinates are distances.)"""
    p = np.asarray(p, dtype=f8)
    disc = np.hypot(*(p - B.pos).T) - B.rb
    e = np.abs(B.local(p)) - B.h
    box = np.where((e <= 0).all(axis=1), e.max(axis=1), np.hypot(*np.maximum(e, 0.0).T))
    return np.where(B.round, disc, box)


def _foot(B, p):
    """Every body's closest point to p (N, 2), and for a box how far p's local coordinates are outside the half extents (N, 2)."""
    l = B.local(p)
    k = np.clip(l, -B.h, B.h)
    box = B.pos + k[:, :1] * B.xv + k[:, 1:] * B.yv
    w = p - B.pos
    with np.errstate(invalid="ignore", divide="ignore"):
        disc = B.pos + w * (B.rb / np.hypot(*w.T))[:, None]
    return np.where(B.round[:, None], disc, box), np.abs(l) - B.h


def overlap(B, c):
    c = np.asarray(c, dtype=np.float32).astype(f8)
    s = sd(B, c[0:2])
    return s <= c[2], np.abs(s - c[2])


class Verdict:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def cast(B, c):
    """The cast {c.x, c.y, r, dx, dy, max_t} (float32 values) against every body."""
    c = np.asarray(c, dtype=np.float32).astype(f8)
    o, r, d, max_t = c[0:2], c[2], c[3:5], c[5]
    f = lambda t: sd(B, o + t[:, None] * d) - r      # noqa: E731
    zero = np.zeros(B.n)
    f0 = f(zero)
    # golden section on [0, max_t], every body at once
    lo, hi = zero.copy(), np.full(B.n, max_t)
    x1, x2 = hi - GOLD * (hi - lo), lo + GOLD * (hi - lo)
    f1, f2 = f(x1), f(x2)
    for _ in range(100):                                                # (0.618^100: below a float64's resolution of any interval here)
        left = f1 < f2                                                  # the minimum lies in [lo, x2]; otherwise in [x1, hi]
        lo, hi = np.where(left, lo, x1), np.where(left, x2, hi)
        xn = np.where(left, hi - GOLD * (hi - lo), lo + GOLD * (hi - lo))
        fn = f(xn)
        x1, x2, f1, f2 = np.where(left, xn, x2), np.where(left, x1, xn), np.where(left, fn, f2), np.where(left, f1, fn)
    cand = np.stack([zero, lo, x1, x2, hi, np.full(B.n, max_t)])
    vals = np.stack([f0, f(lo), f1, f2, f(hi), f(np.full(B.n, max_t))])
    pick = vals.argmin(axis=0)
    tmin, fmin = cand[pick, np.arange(B.n)], vals[pick, np.arange(B.n)]
    inside = f0 <= 0
    hit = inside | (fmin <= 0)
    # the first root: f(a) > 0 >= f(b)
    a, b = zero.copy(), np.where(hit & ~inside, tmin, 0.0)
    for _ in range(70):
        mid = 0.5 * (a + b)
        neg = f(mid) <= 0
        a, b = np.where(neg, a, mid), np.where(neg, mid, b)
    t = np.where(hit, np.where(inside, 0.0, b), np.nan)
    at = o + np.where(hit, t, 0.0)[:, None] * d
    foot, outside = _foot(B, at)
    n = at - foot
    with np.errstate(invalid="ignore", divide="ignore"):
        n = n / np.hypot(*n.T)[:, None]
    normal = np.where((hit & ~inside)[:, None], n, np.nan)
    clearance = np.where(hit, np.where(inside, -f0, np.minimum(f0, -fmin)), fmin)
    return Verdict(hit=hit, t=t, inside=inside, normal=normal, clearance=clearance, outside=outside, r=r)


def closest(v):
    if not v.hit.any():
        return -1
    t = np.where(v.hit, v.t, np.inf)
    return int(np.flatnonzero(t == t.min())[0])


def unit(B, q, v=None):
    """u = 2^-24 * scale per body: what a float32 of the size the query handles can carry.  q: a circle (3) or a cast (6)."""
    q = np.asarray(q, dtype=np.float32).astype(f8)
    scale = np.maximum(np.maximum(1.0, max(np.hypot(*q[0:2]), q[2])), np.maximum(np.hypot(*B.pos.T), B.size))
    if v is not None:
        scale = np.maximum(scale, np.where(v.hit, v.t, 0.0) * np.hypot(*q[3:5]))
    return scale * 2.0 ** -24


def rho(B, c, v, b):
    """The radius a normal's error is measured on (see the module's text); a hit within NEAR u of a box's corner region counts as there."""
    if B.round[b]:
        return v.r + B.rb[b]
    u = unit(B, c, v)[b]
    return v.r if (v.outside[b] > -NEAR * u).all() else B.size[b] + v.r


def deviation(B, c, v, b, t, normal):
    """The measures of a float32 answer {t, normal} of cast c for body b, which the judge's Verdict v says is hit.  In lengths:
      hit      |t - t_judge| * |d|
      normal   the angle between normal and the judge's, * rho   (0 where the judge has no normal: the cast starts overlapping)
      length   | |normal| - 1 | * rho"""
    c = np.asarray(c, dtype=np.float32).astype(f8)
    out = {"hit": abs(f8(t) - v.t[b]) * float(np.hypot(*c[3:5])), "normal": 0.0, "length": 0.0}
    want = v.normal[b]
    if not np.isnan(want).any():
        n = np.asarray(normal, dtype=f8)
        size = rho(B, c, v, b)
        out["length"] = abs(float(np.hypot(*n)) - 1.0) * size
        out["normal"] = abs(float(np.arctan2(n[0] * want[1] - n[1] * want[0], n @ want))) * size
    return out
