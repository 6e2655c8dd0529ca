"""The float64 judge of tests/circle_spec.py: the contact of a pair with a circle computed in float64 from the same float32 records, and
the measures a float32 result is held to.  It shares no code with the specification: it works in the box's frame with the closest
point on the box and never looks at the spec's intermediate values.

The judge gives, for a pair: whether the shapes touch, the signed depth (>= 0: penetration along the normal), the unit normal from
body 2 towards body 1 (None where it is not defined: concentric circles, a centre inside the box at equal depth from two faces), and
the distances of a point from the two surfaces.  deviation() measures a float32 contact {p1, p2, n} against it:
  length   | |n| - 1 |
  normal   the angle between n and the judge's normal, in radians (0 where the judge has none)
  depth    | (p2 - p1) . n - depth | / scale
  surface  the larger distance of p1 from body 1's surface and of p2 from body 2's, / scale
with scale = the largest of 1, the bodies' coordinates and their sizes (a float32 coordinate of that size carries 6e-8 * scale)."""
import numpy as np

BOX, CIRCLE = 0, 1


class Body:
    def __init__(self, rec, kind):
        f = np.float64
        self.pos = np.array([f(rec["pos"]["x"]), f(rec["pos"]["y"])])
        self.xv = np.array([f(rec["xv"]["x"]), f(rec["xv"]["y"])])
        self.yv = np.array([f(rec["yv"]["x"]), f(rec["yv"]["y"])])
        self.h = np.array([f(rec["geom_size"]["x"]), f(rec["geom_size"]["y"])])
        self.kind = int(kind)

    def local(self, p):
        """p in the body's frame.  The float32 frame is orthonormal to a few ulp only: solved, not projected."""
        m = np.array([[self.xv[0], self.yv[0]], [self.xv[1], self.yv[1]]])
        return np.linalg.solve(m, np.asarray(p, dtype=np.float64) - self.pos)

    def surface_distance(self, p):
        """|distance| of the world point p from the body's surface."""
        if self.kind == CIRCLE:
            return abs(np.hypot(*(np.asarray(p, dtype=np.float64) - self.pos)) - self.h[0])
        q = self.local(p)
        # the frame's axes have length 1 to float32 accuracy, so local coordinates are distances
        d = np.abs(q) - self.h
        if (d <= 0).all():
            return float(-d.max())
        return float(np.hypot(*np.maximum(d, 0.0)))


def scale(b1, b2):
    return float(max(1.0, np.abs(b1.pos).max(), np.abs(b2.pos).max(), b1.h.max(), b2.h.max()))


def judge(rec1, kind1, rec2, kind2):
    """{"depth": signed depth, "normal": unit vector from body 2 towards body 1 or None, "touching": depth >= 0}"""
    b1, b2 = Body(rec1, kind1), Body(rec2, kind2)
    if kind1 == CIRCLE and kind2 == CIRCLE:
        d = b1.pos - b2.pos
        l = float(np.hypot(*d))
        depth = b1.h[0] + b2.h[0] - l
        normal = d / l if l > 0 else None
    else:
        c, b, sign = (b1, b2, 1.0) if kind1 == CIRCLE else (b2, b1, -1.0)
        assert c.kind == CIRCLE and b.kind == BOX
        q = b.local(c.pos)
        inside = np.abs(q) - b.h                                         # both <= 0: the centre is inside or on the box
        m = np.array([[b.xv[0], b.yv[0]], [b.xv[1], b.yv[1]]])
        if (inside <= 0).all():
            face = int(np.argmax(inside))
            depth = c.h[0] - inside[face]
            tie = inside[0] == inside[1]
            local_n = np.zeros(2)
            local_n[face] = -1.0 if q[face] < 0 else 1.0
            normal = None if tie else sign * (m @ local_n)
        else:
            e = q - np.clip(q, -b.h, b.h)
            l = float(np.hypot(*e))
            depth = c.h[0] - l
            normal = sign * (m @ (e / l))
        if normal is not None:
            normal = normal / np.hypot(*normal)
    return {"depth": float(depth), "normal": normal, "touching": depth >= 0, "bodies": (b1, b2)}


def deviation(verdict, p1, p2, n):
    """The four measures of a float32 contact against judge()'s verdict."""
    b1, b2 = verdict["bodies"]
    p1, p2, n = (np.asarray(v, dtype=np.float64) for v in (p1, p2, n))
    s = scale(b1, b2)
    length = abs(float(np.hypot(*n)) - 1.0)
    if verdict["normal"] is None:
        angle = 0.0
    else:
        u = n / np.hypot(*n)
        angle = abs(float(np.arctan2(u[0] * verdict["normal"][1] - u[1] * verdict["normal"][0], u @ verdict["normal"])))
    depth = abs(float((p2 - p1) @ n) - verdict["depth"]) / s
    surface = max(b1.surface_distance(p1), b2.surface_distance(p2)) / s
    return {"length": length, "normal": angle, "depth": depth, "surface": surface}
