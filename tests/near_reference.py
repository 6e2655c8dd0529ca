"""The float64 judge of the nearest-body query (include/phyx_amd.h, QUERIES: phx_world_query_nearest): how far a point is from every
body, where the body's closest surface point (the foot) is and which way the surface faces there, computed in float64 from the same
float32 records, kinds and polygons, and the measures a float32 answer is held to.  It shares no code and no method with
tests/near_spec.py: a point's frame coordinates are found by solving against the float32 frame (not by projecting on it, as
round_query_reference.Bodies.local), a box's and a capsule's foot by clipping them, and a polygon knows no normals and no regions: its
foot is the closest of the closest points of its edges, taken as segments, and the point is inside iff it is left of every edge.

  Bodies(records, kinds, polys)   the float64 columns
  near(B, p)                      Verdict per body: sd, foot, normal, region ("face", "corner", "round"), medial (inside: how far the
                                  point is from where foot and normal jump: the second smallest face depth minus the smallest, the
                                  distance from a circle's centre or a capsule's core; outside in a corner's or a vertex's region
                                  the distance from its tip, where the inside's medial set meets the surface; inf elsewhere)
  unit(B, p, v)                   u = 2^-24 * the largest of 1, |p|, |pos|, the sizes and |sd|, per body
  deviation(B, p, v, b, hit)      the measures of a float32 answer for body b, in lengths:
      distance   |D - sd|
      point      |point - foot|
      normal     the angle between the normals times a radius: max(|sd|, NEAR u) in a corner, vertex or round region (the normal turns
                 by 1 / |sd| per unit of length there, for any rule), the body's size where the normal is a face's
      length     | |normal| - 1 | on the same radius"""
import numpy as np

BOX, CIRCLE, CAPSULE, POLYGON = 0, 1, 2, 3
KINDS = ("box", "disc", "capsule", "polygon")
f8 = np.float64
NEAR = 32.0             # a verdict this many u from changing may be excused (query_reference.NEAR)
MEASURES = ("distance", "point", "normal", "length")


class Bodies:
    def __init__(self, records, kinds, polys=None):
        b = np.asarray(records)
        col = lambda name: np.stack([b[name]["x"].astype(f8), b[name]["y"].astype(f8)], axis=1)      # noqa: E731
        self.n = len(b)
        self.pos, self.xv, self.yv, self.h = col("pos"), col("xv"), col("yv"), col("geom_size")
        self.kind = np.zeros(self.n, dtype=np.int64) if kinds is None else np.asarray(kinds).astype(np.int64)
        self.size = self.h.max(axis=1)
        self.det = self.xv[:, 0] * self.yv[:, 1] - self.xv[:, 1] * self.yv[:, 0]
        self.verts = {int(i): np.asarray(polys[i]["v"], dtype=np.float32).astype(f8).reshape(8, 2)[:int(polys[i]["count"])]
                      for i in np.flatnonzero(self.kind == POLYGON)}

    def local(self, p):
        """p (2,) in every body's frame: the solution of pos + a*xv + b*yv = p."""
        q = np.asarray(p, dtype=f8) - self.pos
        a = (q[:, 0] * self.yv[:, 1] - q[:, 1] * self.yv[:, 0]) / self.det
        b = (self.xv[:, 0] * q[:, 1] - self.xv[:, 1] * q[:, 0]) / self.det
        return np.stack([a, b], axis=1)

    def world(self, l):
        """Frame coordinates (N, 2) in the world."""
        return self.pos + l[:, :1] * self.xv + l[:, 1:] * self.yv

    def turn(self, d):
        """Frame directions (N, 2) in the world, at unit length."""
        w = d[:, :1] * self.xv + d[:, 1:] * self.yv
        with np.errstate(invalid="ignore", divide="ignore"):
            return w / np.hypot(*w.T)[:, None]


class Verdict:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _second_gap(depths):
    """The second smallest of each row minus the smallest."""
    s = np.sort(depths, axis=1)
    return s[:, 1] - s[:, 0]


def _boxes(B, l):
    e = np.abs(l) - B.h
    inside = (e <= 0).all(axis=1)
    out = np.maximum(e, 0.0)
    sd = np.where(inside, e.max(axis=1), np.hypot(*out.T))
    sign = np.where(l < 0, -1.0, 1.0)
    axis = np.argmax(e, axis=1)                                            # inside: the face of the smallest depth
    k = np.clip(l, -B.h, B.h)
    rows = np.arange(B.n)
    k_in = l.copy()
    k_in[rows, axis] = (sign * B.h)[rows, axis]
    d_in = np.zeros_like(l)
    d_in[rows, axis] = sign[rows, axis]
    d_out = l - k
    foot = B.world(np.where(inside[:, None], k_in, k))
    normal = B.turn(np.where(inside[:, None], d_in, d_out))
    corner = ~inside & (out > 0).all(axis=1)
    depths = np.concatenate([B.h - l, B.h + l], axis=1)
    medial = np.where(inside, _second_gap(depths), np.inf)
    return sd, foot, normal, corner, medial


def _discs(B, p):
    w = p - B.pos
    l = np.hypot(*w.T)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = w / l[:, None]
    sd = l - B.h[:, 0]
    return sd, B.pos + n * B.h[:, :1], n, np.where(sd <= 0, l, np.inf)


def _capsules(B, l):
    r, a = B.h[:, 1], B.h[:, 0] - B.h[:, 1]
    qu = np.clip(l[:, 0], -a, a)
    g = np.stack([l[:, 0] - qu, l[:, 1]], axis=1)
    length = np.hypot(*g.T)
    sd = length - r
    n = B.turn(g)
    core = B.pos + qu[:, None] * B.xv
    return sd, core + n * r[:, None], n, np.where(sd <= 0, length, np.inf)


def _polygon(v, p):
    """One polygon in its frame: (sd, foot, direction of the normal, whether the foot is a vertex, medial)."""
    w = np.roll(v, -1, axis=0)
    e = w - v
    t = np.clip(((p - v) * e).sum(axis=1) / (e * e).sum(axis=1), 0.0, 1.0)
    c = v + t[:, None] * e                                                  # every edge's closest point, as a segment
    d = np.hypot(*(p - c).T)
    k = int(np.argmin(d))
    inside = bool(((e[:, 0] * (p - v)[:, 1] - e[:, 1] * (p - v)[:, 0]) >= 0).all())
    vertex = bool(t[k] <= 0.0 or t[k] >= 1.0)
    if inside:
        lines = np.abs(e[:, 0] * (p - v)[:, 1] - e[:, 1] * (p - v)[:, 0]) / np.hypot(*e.T)      # the depths to the edges' lines
        s = np.sort(lines)
        return -d[k], c[k], c[k] - p, False, s[1] - s[0]
    return d[k], c[k], p - c[k], vertex, np.inf


def near(B, p):
    """Every body against the point p (2,)."""
    p = np.asarray(p, dtype=np.float32).astype(f8)[:2]
    l = B.local(p)
    sd, foot, normal, corner, medial = _boxes(B, l)
    region = np.where(corner, "corner", "face").astype(object)
    for kind, cols in ((CIRCLE, _discs(B, p)), (CAPSULE, _capsules(B, l))):
        m = B.kind == kind
        sd, foot, normal, medial = np.where(m, cols[0], sd), np.where(m[:, None], cols[1], foot), np.where(m[:, None], cols[2], normal), np.where(m, cols[3], medial)
        region[m] = "round"
    for b, v in B.verts.items():
        s, c, d, vertex, med = _polygon(v, l[b])
        sd[b], medial[b], region[b] = s, med, "corner" if vertex else "face"
        foot[b] = B.pos[b] + c[0] * B.xv[b] + c[1] * B.yv[b]
        w = d[0] * B.xv[b] + d[1] * B.yv[b]
        with np.errstate(invalid="ignore", divide="ignore"):
            normal[b] = w / np.hypot(*w)
    medial = np.where((region == "corner") & (sd > 0), sd, medial)
    return Verdict(p=p, sd=sd, foot=foot, normal=normal, region=region, medial=medial)


def unit(B, p, v):
    p = np.asarray(p, dtype=np.float32).astype(f8)[:2]
    scale = np.maximum.reduce([np.ones(B.n), np.full(B.n, np.hypot(*p)), np.hypot(*B.pos.T), B.size, np.abs(v.sd)])
    return 2.0 ** -24 * scale


def deviation(B, p, v, b, hit):
    """The measures of the float32 answer `hit` (a near_hit_dtype record naming body b), in lengths."""
    u = unit(B, p, v)[b]
    n = np.asarray(hit["normal"], dtype=f8)
    radius = B.size[b] if v.region[b] == "face" else max(abs(v.sd[b]), NEAR * u)
    cross = n[0] * v.normal[b, 1] - n[1] * v.normal[b, 0]
    dot = n[0] * v.normal[b, 0] + n[1] * v.normal[b, 1]
    return {"distance": abs(float(hit["distance"]) - v.sd[b]),
            "point": float(np.hypot(*(np.asarray(hit["point"], dtype=f8) - v.foot[b]))),
            "normal": abs(float(np.arctan2(abs(cross), dot))) * radius,
            "length": abs(float(np.hypot(*n)) - 1.0) * radius}
