"""The float64 judge of the point and ray queries (include/phyx_amd.h, QUERIES): what a point or a ray meets, computed in float64 from
the same float32 records and kinds, and the measures a float32 answer is held to.  It shares no code and no intermediate value with
tests/query_spec.py, tests/shape_query_spec.py or tests/circle_spec.py: a box is the parallelogram pos + a*xv + b*yv, |a| <= h.x,
|b| <= h.y, met in world space by clipping against its four edges' half-planes, not by slabs in the body's frame; a disc is met by
projecting its centre onto the ray's line, not by a quadratic in t.  Oriented boxes and casts keep their judge in
tests/test_shape_queries_cpu.py.

Everything is vectorised over the bodies: one query against all of them.
  Bodies                   the float64 columns of the records
  point(B, p)              the signed distance of p from every body's surface (< 0: inside)
  ray(B, r)                Verdict: hit, the entry t, the outward normal of what is entered (NaN where the origin is inside), how far
                           the entry is from a box's corner (there the entered edge is a tie: deviation() leaves the normal out
                           within NEAR u of one), the clearance, per body
  closest(v)               the index of the closest hit of a Verdict (smallest t, then the lowest index), -1 if none
  unit(B, r, v)            u = 2^-24 * scale per body, scale = the largest of 1, |o|, |pos|, the sizes and t*|d|
  deviation(B, r, v, b, t, normal, point)   the measures of a float32 answer {t, normal, point} for body b, in lengths

The clearance is how far, in length, the ray is from changing its verdict on a body: the smallest of the depth of the ray's line in
the body (or the distance it passes it at), the length from the origin to the exit and the length from the entry to the max_t end, each
as far as it bears on the verdict (see _clearance)."""
import numpy as np

BOX, CIRCLE = 0, 1
f8 = np.float64


class Bodies:
    def __init__(self, records, kinds):
        b = np.asarray(records)
        col = lambda name: np.stack([b[name]["x"].astype(f8), b[name]["y"].astype(f8)], axis=1)      # noqa: E731
        self.n = len(b)
        self.pos, self.xv, self.yv, self.h = col("pos"), col("xv"), col("yv"), col("geom_size")
        self.round = np.asarray(kinds).astype(np.int64) == CIRCLE
        self.r = self.h[:, 0]
        self.size = np.where(self.round, self.r, self.h.max(axis=1))

    def local(self, p):
        """p (2,) or (N, 2) in every body's frame.  The float32 frame is orthonormal to a few ulp only: solved (Cramer), not projected."""
        q = np.asarray(p, dtype=f8) - self.pos
        det = self.xv[:, 0] * self.yv[:, 1] - self.xv[:, 1] * self.yv[:, 0]
        a = (q[:, 0] * self.yv[:, 1] - q[:, 1] * self.yv[:, 0]) / det
        b = (self.xv[:, 0] * q[:, 1] - self.xv[:, 1] * q[:, 0]) / det
        return np.stack([a, b], axis=1)


def point(B, p):
    """The signed distance of the world point p from every body's surface: < 0 inside, > 0 outside.  (A frame's axes have length 1 to
    float32 accuracy, so a box's local coordinates are distances.)"""
    p = np.asarray(p, dtype=f8)
    disc = np.hypot(*(p - B.pos).T) - B.r
    d = np.abs(B.local(p)) - B.h
    outside = np.hypot(*np.maximum(d, 0.0).T)
    box = np.where((d <= 0).all(axis=1), d.max(axis=1), outside)
    return np.where(B.round, disc, box)


class Verdict:
    """Per body: hit, t (the entry clamped to >= 0; NaN on a miss), inside (the origin is inside or on the body), normal (N, 2), clearance,
    tin / tout of the ray's LINE in the body (NaN where the line misses it), and corner: the length between the last two edges a ray
    enters a box through (inf for a disc or a single edge; near 0 the entered edge, and with it the normal, is a tie)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _clearance(depth, tin, tout, max_t, dlen):
    """depth: of the line in the body (< 0: the distance it passes at).  A line that misses: -depth.  A line that hits: the ray hits iff
    tout >= 0 and tin <= max_t; a hit is as far from a miss as the smallest of the depth and the two lengths, a miss as far from a hit
    as the largest violated length, and no further than the depth (a shallow chord's ends move fast)."""
    back, ahead = tout * dlen, (max_t - tin) * dlen
    hit = (depth >= 0) & (back >= 0) & (ahead >= 0)
    with np.errstate(invalid="ignore"):
        miss_by = np.maximum(np.where(back < 0, -back, 0.0), np.where(ahead < 0, -ahead, 0.0))
        c = np.where(hit, np.minimum(depth, np.minimum(back, ahead)), np.minimum(np.abs(depth), miss_by))
    return hit, np.where(depth < 0, -depth, c)


def _ray_discs(B, o, d, max_t):
    dlen = np.hypot(*d)
    u = d / dlen
    w = B.pos - o
    along = w @ u                                                     # the centre's foot on the line, as a length from o
    foot = o + along[:, None] * u
    dist = np.hypot(*(foot - B.pos).T)
    depth = B.r - dist
    with np.errstate(invalid="ignore"):
        half = np.sqrt(B.r * B.r - dist * dist)
    tin, tout = (along - half) / dlen, (along + half) / dlen
    hit, clear = _clearance(depth, tin, tout, max_t, dlen)
    inside = hit & (tin <= 0)
    t = np.where(hit, np.maximum(tin, 0.0), np.nan)
    at = o + t[:, None] * d
    normal = np.where((hit & ~inside)[:, None], (at - B.pos) / B.r[:, None], np.nan)
    return Verdict(hit=hit, t=t, inside=inside, normal=normal, clearance=clear, tin=tin, tout=tout, corner=np.full(B.n, np.inf))


def _ray_boxes(B, o, d, max_t):
    dlen = np.hypot(*d)
    side = np.array([-d[1], d[0]]) / dlen                              # the line's unit normal
    # the four edges: a point on each and its outward unit normal (perpendicular to the edge's direction, pointing away from pos)
    tin = np.full(B.n, -np.inf)
    tout = np.full(B.n, np.inf)
    entered = np.full(B.n, -1)
    second = np.full(B.n, -np.inf)                                     # the entering crossing before the last: a corner when close
    apart = np.zeros(B.n)                                              # > 0: parallel to an edge and outside it by this much
    normals = []
    for k, (axis, other, s) in enumerate(((B.xv * B.h[:, :1], B.yv, 1.0), (B.xv * B.h[:, :1], B.yv, -1.0),
                                           (B.yv * B.h[:, 1:], B.xv, 1.0), (B.yv * B.h[:, 1:], B.xv, -1.0))):
        on = B.pos + s * axis
        n = np.stack([other[:, 1], -other[:, 0]], axis=1)
        n = n / np.hypot(*n.T)[:, None]
        n = n * np.sign(np.einsum("ni,ni->n", n, s * axis))[:, None]
        normals.append(n)
        f0 = np.einsum("ni,ni->n", n, o - on)                           # the origin's distance outside this edge's line
        rate = n @ d
        with np.errstate(divide="ignore", invalid="ignore"):
            tc = -f0 / rate
        enter, leave = rate < 0, rate > 0
        later = enter & (tc > tin)
        second = np.where(later, tin, np.where(enter, np.maximum(second, tc), second))
        entered = np.where(later, k, entered)
        tin = np.where(later, tc, tin)
        tout = np.where(leave & (tc < tout), tc, tout)
        apart = np.maximum(apart, np.where(rate == 0, f0, 0.0))
    # the depth of the line in the box: the corners' distances from the line lie on both sides of 0 iff it passes through
    c = []
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            c.append((B.pos + sx * B.xv * B.h[:, :1] + sy * B.yv * B.h[:, 1:] - o) @ side)
    c = np.stack(c, axis=1)
    depth = np.minimum(c.max(axis=1), -c.min(axis=1))
    through = (depth >= 0) & (apart <= 0) & (tin <= tout)
    tin, tout = np.where(through, tin, np.nan), np.where(through, tout, np.nan)
    hit, clear = _clearance(np.where(through, depth, -np.abs(depth)), tin, tout, max_t, dlen)
    inside = hit & (tin <= 0)
    t = np.where(hit, np.maximum(tin, 0.0), np.nan)
    normal = np.full((B.n, 2), np.nan)
    for k, n in enumerate(normals):
        normal = np.where((hit & ~inside & (entered == k))[:, None], n, normal)
    with np.errstate(invalid="ignore"):
        corner = np.where(hit & ~inside, (tin - second) * dlen, np.inf)
    return Verdict(hit=hit, t=t, inside=inside, normal=normal, clearance=clear, tin=tin, tout=tout, corner=corner)


def ray(B, r):
    """The ray {ox, oy, dx, dy, max_t} (float32 values) against every body."""
    r = np.asarray(r, dtype=np.float32).astype(f8)
    o, d, max_t = r[0:2], r[2:4], r[4]
    a, b = _ray_discs(B, o, d, max_t), _ray_boxes(B, o, d, max_t)
    pick = lambda x, y: np.where(B.round if x.ndim == 1 else B.round[:, None], x, y)      # noqa: E731
    return Verdict(**{k: pick(getattr(a, k), getattr(b, k)) for k in ("hit", "t", "inside", "normal", "clearance", "tin", "tout", "corner")})


def closest(v):
    if not v.hit.any():
        return -1
    t = np.where(v.hit, v.t, np.inf)
    return int(np.flatnonzero(t == t.min())[0])


def unit(B, r, v=None):
    """u = 2^-24 * scale per body: what a float32 of the size the query handles can carry."""
    r = np.asarray(r, dtype=np.float32).astype(f8)
    o = np.hypot(*r[0:2]) if len(r) >= 2 else 0.0
    scale = np.maximum(np.maximum(1.0, o), np.maximum(np.hypot(*B.pos.T), B.size))
    if v is not None:
        scale = np.maximum(scale, np.where(v.hit, v.t, 0.0) * np.hypot(*r[2:4]))
    return scale * 2.0 ** -24


MEASURES = ("hit", "length", "angle", "surface")
NEAR = 32.0             # a verdict (or an entered edge) this many u from changing may be excused


def deviation(B, r, v, b, t, normal, point_):
    """The measures of a float32 answer {t, normal, point} of ray r for body b, which the judge's Verdict v says is hit.  In lengths:
      hit      the distance of o + t*d from the judge's hit point
      length   | |normal| - 1 | * size        (size: the radius, a box's larger half extent; 0 where the judge has no normal:
               the origin inside, a corner within NEAR u)
      angle    the angle between normal and the judge's, * size
      surface  the distance of the returned point from the body's surface (0 when the origin is inside: the point is the origin)"""
    r = np.asarray(r, dtype=np.float32).astype(f8)
    o, d = r[0:2], r[2:4]
    out = {"hit": float(np.hypot(*((o + f8(t) * d) - (o + v.t[b] * d)))), "length": 0.0, "angle": 0.0, "surface": 0.0}
    want = v.normal[b]
    if not np.isnan(want).any() and v.corner[b] > NEAR * unit(B, r, v)[b]:
        n = np.asarray(normal, dtype=f8)
        out["length"] = abs(float(np.hypot(*n)) - 1.0) * B.size[b]
        out["angle"] = abs(float(np.arctan2(n[0] * want[1] - n[1] * want[0], n @ want))) * B.size[b]
    if not v.inside[b]:
        out["surface"] = abs(float(point(B, np.asarray(point_, dtype=f8))[b]))
    return out
